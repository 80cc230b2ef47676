"""Probe: what sending a ragged batch of torch tensors in HBM as one List message costs against
the struct send of the same values, which this tree contains unchanged.

Records, src and sink on GPU 0 of one process:

  c3                {x, y, z: columns of a (1000000, 3) float32, intensity: uint8}, B = 16
  detector_100      {bbox: out[:, :4], conf: out[:, 4], cls: out[:, 5]} of a (100, 6) float32, B = 8
  detector_100000   the same of a (100000, 6) float32, B = 8
  scan_16, scan_4096, scan_1048576
                    B single bytes cut into B lists of one: next to nothing for the fields' share,
                    so the launch's time is the scan share's (ragged_dev only)

Modes, interleaved in `--rounds` rounds of `--messages` synchronous sends each:

  struct       node.send_output("s", {name: view, ..}): the yardstick (runs in a tree without
               ragged sends too: `--modes struct`)
  ragged_dev   node.send_output("s", tensor.ragged(values, lengths=<int64 tensor in HBM>)): the
               struct send's work plus one more DLPack handshake and one more workgroup
  ragged_host  the same with lengths=<Python list>: plus one small copy on the fill stream

each as the time of the synchronous call of one message (p10 / p50 / p90 us over the round; the
sink drains after the clock stops).  One JSON line per (record, mode, round) goes to `--out`.

    python scripts/tensor_list_probe.py --out profiles/tensor_list_probe.jsonl

The launch's own device time comes from a kernel trace of the same script, a run of its own
without counters, read back with `--trace-db` (same `--messages`, `--warmup`, `--records` and
`--modes`):

    rocprofv3 --kernel-trace --stats -d OUT -o list -- \\
        python scripts/tensor_list_probe.py --messages 50 --rounds 1 --out OUT/probe.jsonl
    python scripts/tensor_list_probe.py --messages 50 --trace-db OUT/list_results.db \\
        --out profiles/tensor_list_probe.jsonl --append

which adds one line per (record, mode): p50 of gather_struct_kernel.
"""
import argparse
import json
import os
import sys
import threading
import time

RECORDS = ("c3", "detector_100", "detector_100000", "scan_16", "scan_4096", "scan_1048576")
MODES = ("struct", "ragged_dev", "ragged_host")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESC = {"nodes": [
    {"id": "src", "path": "dynamic", "outputs": ["s"]},
    {"id": "dst", "path": "dynamic", "inputs": {"s": {"source": "src/s", "queue_size": 10}}},
]}


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))] / 1e3


def split(n, b):
    """b lengths that sum to n, unequal, one of them empty."""
    ln = [n // b] * b
    ln[0] += n - sum(ln)
    if b > 2:
        ln[1] += ln[2]
        ln[2] = 0
    return ln


def records(torch, names):
    """name -> (values, lengths as a list, modes that apply)."""
    dev = torch.device("cuda", 0)
    out = {}
    for name in names:
        if name == "c3":
            p = torch.rand((1000000, 3), dtype=torch.float32, device=dev)
            i = torch.randint(0, 255, (1000000,), dtype=torch.uint8, device=dev)
            out[name] = ({"x": p[:, 0], "y": p[:, 1], "z": p[:, 2], "intensity": i},
                         split(1000000, 16), MODES)
        elif name.startswith("detector_"):
            n = int(name.split("_")[1])
            o = torch.rand((n, 6), dtype=torch.float32, device=dev)
            out[name] = ({"bbox": o[:, :4], "conf": o[:, 4], "cls": o[:, 5]}, split(n, 8), MODES)
        else:
            b = int(name.split("_")[1])
            v = torch.zeros((b,), dtype=torch.uint8, device=dev)
            out[name] = ({"v": v}, [1] * b, ("ragged_dev",))
    return out


def trace_rows(db, plan, messages, warmup):
    """p50 of gather_struct_kernel per (record, mode) that launches it, from the dispatches in
    start order: the probe's own order, warm-up first."""
    import sqlite3
    c = sqlite3.connect(db)
    disp = [d for (d,) in c.execute("select end - start from kernels where name like "
                                    "'%gather_struct_kernel%' order by start")]
    per = warmup + messages
    rows = []
    for name, mode in plan:
        m, disp = disp[:per][warmup:], disp[per:]
        if len(m) != messages:
            raise SystemExit(f"{name} {mode}: {len(m)} launches in the trace, {messages} expected")
        rows.append({"record": name, "mode": mode + "_kernel_trace", "messages": messages,
                     "kernel_us_p10": pct(m, 0.1), "kernel_us_p50": pct(m, 0.5),
                     "kernel_us_p90": pct(m, 0.9)})
    if disp:
        raise SystemExit(f"{len(disp)} launches left over")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_list_probe.jsonl"))
    ap.add_argument("--messages", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--records", default=",".join(RECORDS))
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--tree", default="", help="a label for the tree that ran, copied into every line")
    ap.add_argument("--trace-db", default="", help="read a rocprofv3 kernel trace of this probe "
                    "(one round) instead of running it")
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    names = [r for r in a.records.split(",") if r]
    modes = [m for m in a.modes.split(",") if m]
    rows = []
    if a.trace_db:
        # every mode launches gather_struct_kernel here: each record has a strided field, and a
        # partition in HBM always takes the launch
        plan = [(n, m) for n in names for m in modes
                if m == "ragged_dev" or not n.startswith("scan_")]
        rows = trace_rows(a.trace_db, plan, a.messages, a.warmup)
    else:
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

                def one(msg):
                    """One message; ns of the synchronous call."""
                    t0 = time.perf_counter_ns()
                    tx.send_output("s", msg)
                    dt = time.perf_counter_ns() - t0
                    ev = rx.next(timeout=60)
                    assert ev["type"] == "INPUT"
                    del ev
                    return dt

                try:
                    recs = records(torch, names)
                    torch.cuda.synchronize()
                    for name in names:
                        vals, ln, applies = recs[name]
                        counts = torch.tensor(ln, dtype=torch.int64, device=torch.device("cuda", 0))
                        torch.cuda.synchronize()
                        msgs = {"struct": lambda: vals,
                                "ragged_dev": lambda: tensor.ragged(vals, lengths=counts),
                                "ragged_host": lambda: tensor.ragged(vals, lengths=ln)}
                        nbytes = sum(v.numel() * v.element_size() for v in vals.values())
                        for rnd in range(a.rounds):
                            for mode in modes:
                                if mode not in applies:
                                    continue
                                if rnd == 0:  # warm up: slots, streams, code objects
                                    for _ in range(a.warmup):
                                        one(msgs[mode]())
                                per = [one(msgs[mode]()) for _ in range(a.messages)]
                                rows.append({"record": name, "mode": mode, "round": rnd, "lists": len(ln),
                                             "bytes": nbytes, "messages": a.messages,
                                             "sync_us_p10": pct(per, 0.1), "sync_us_p50": pct(per, 0.5),
                                             "sync_us_p90": pct(per, 0.9)})
                                if a.tree:
                                    rows[-1]["tree"] = a.tree
                                print(json.dumps(rows[-1]), flush=True)
                finally:
                    for k in n.values():
                        k.close()
        finally:
            lch.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    if a.trace_db:
        for r in rows:
            print(json.dumps(r))


if __name__ == "__main__":
    main()
