"""Probe: what sending a record of strided torch tensors in HBM as one Struct message costs against
sending the same views as separate messages, which is what a tree without struct sends can do
(DESIGN §4).

Records, src and sink on GPU 0 of one process:

  detector_100      {bbox: out[:, :4], conf: out[:, 4], cls: out[:, 5]} of a (100, 6) float32
  detector_100000   the same of a (100000, 6) float32
  frame             {rgb: (1080, 1920, 3) uint8 -> CHW, depth: a (1080, 1920) crop of a
                    (1200, 2000) float32}, each with unsqueeze(0): a struct of length 1

Modes, interleaved in `--rounds` rounds of `--messages` synchronous sends each:

  struct     node.send_output("s", {name: view, ..}): one plan, one slot, one launch of
             gather_struct_kernel, one descriptor, one event at the sink
  separate   node.send_output(name, view) per field on outputs of their own: n of each

each as the time of the synchronous call(s) of one record (p10 / p50 / p90 us over the round; the
sink drains after the clock stops).  One JSON line per (record, mode, round) goes to `--out`.

    python scripts/tensor_struct_probe.py --out profiles/tensor_struct_probe.jsonl

The kernels' own device times come from a kernel trace of the same script, a run of its own
without counters, read back with `--trace-db` (same `--messages`, `--warmup` and `--records`):

    rocprofv3 --kernel-trace --stats -d OUT -o struct -- \\
        python scripts/tensor_struct_probe.py --messages 50 --rounds 1 --out OUT/probe.jsonl
    python scripts/tensor_struct_probe.py --messages 50 --trace-db OUT/struct_results.db \\
        --out profiles/tensor_struct_probe.jsonl --append

which adds one line per record: p50 of gather_struct_kernel against p50 of the sum of the
single-view gather kernels of one record.
"""
import argparse
import json
import os
import sys
import threading
import time

RECORDS = ("detector_100", "detector_100000", "frame")
FIELDS = {"detector_100": 3, "detector_100000": 3, "frame": 2}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESC = {"nodes": [
    {"id": "src", "path": "dynamic", "outputs": ["s", "f0", "f1", "f2"]},
    {"id": "dst", "path": "dynamic",
     "inputs": {k: {"source": "src/" + k, "queue_size": 10} for k in ("s", "f0", "f1", "f2")}},
]}


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))] / 1e3


def records(torch):
    dev = torch.device("cuda", 0)
    out = {}
    for n in (100, 100000):
        o = torch.rand((n, 6), dtype=torch.float32, device=dev)
        out[f"detector_{n}"] = {"bbox": o[:, :4], "conf": o[:, 4], "cls": o[:, 5]}
    frame = torch.randint(0, 255, (1080, 1920, 3), dtype=torch.uint8, device=dev)
    depth = torch.rand((1200, 2000), dtype=torch.float32, device=dev)
    out["frame"] = {"rgb": frame.permute(2, 0, 1).unsqueeze(0),
                    "depth": depth[60:1140, 40:1960].unsqueeze(0)}
    return out


def trace_rows(db, names, messages, warmup):
    """Per record: p50 of gather_struct_kernel and of the summed single-view gathers of one
    record, from the dispatches in start order (the probe's own order: per record the struct
    sends, then the separate ones, warm-up first)."""
    import sqlite3
    c = sqlite3.connect(db)
    disp = list(c.execute("select name, end - start from kernels where name like '%gather_%kernel%' "
                          "order by start"))
    multi = [d for name, d in disp if "gather_struct_kernel" in name]
    single = [d for name, d in disp if "gather_struct_kernel" not in name]
    per = warmup + messages
    rows = []
    for name in names:
        n = FIELDS[name]
        m, multi = multi[:per][warmup:], multi[per:]
        s, single = single[:per * n], single[per * n:]
        sums = [sum(s[i * n:(i + 1) * n]) for i in range(per)][warmup:]
        if len(m) != messages or len(sums) != messages:
            raise SystemExit(f"{name}: {len(m)} struct and {len(sums)} separate records in the trace, "
                             f"{messages} expected")
        rows.append({"record": name, "mode": "kernel_trace", "fields": n, "messages": messages,
                     "struct_kernel_us_p50": pct(m, 0.5), "separate_kernels_us_p50": pct(sums, 0.5)})
    if multi or single:
        raise SystemExit(f"{len(multi)} struct and {len(single)} single dispatches left over")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_struct_probe.jsonl"))
    ap.add_argument("--messages", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--records", default=",".join(RECORDS))
    ap.add_argument("--trace-db", default="", help="read a rocprofv3 kernel trace of this probe "
                    "(one round) instead of running it")
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    names = [r for r in a.records.split(",") if r]
    rows = []
    if a.trace_db:
        rows = trace_rows(a.trace_db, names, a.messages, a.warmup)
    else:
        import torch  # before dora_amd: one HIP runtime for both (dora_amd/node.py)
        sys.path.insert(0, ROOT)
        from dora_amd import launcher as launcher_mod
        lch = launcher_mod.Launcher()  # before HIP is initialised here
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

                def drain(count):
                    for _ in range(count):
                        ev = rx.next(timeout=60)
                        assert ev["type"] == "INPUT"
                        del ev

                def one(mode, rec):
                    """One record; ns of the synchronous call(s)."""
                    t0 = time.perf_counter_ns()
                    if mode == "struct":
                        tx.send_output("s", rec)
                    else:
                        for k, v in enumerate(rec.values()):
                            tx.send_output(f"f{k}", v)
                    dt = time.perf_counter_ns() - t0
                    drain(1 if mode == "struct" else len(rec))
                    return dt

                try:
                    recs = records(torch)
                    torch.cuda.synchronize()
                    for name in names:
                        rec = recs[name]
                        nbytes = sum(v.numel() * v.element_size() for v in rec.values())
                        for rnd in range(a.rounds):
                            for mode in ("struct", "separate"):
                                if rnd == 0:  # warm up: slots, streams, code objects
                                    for _ in range(a.warmup):
                                        one(mode, rec)
                                per = [one(mode, rec) for _ in range(a.messages)]
                                rows.append({"record": name, "mode": mode, "round": rnd, "fields": len(rec),
                                             "bytes": nbytes, "messages": a.messages,
                                             "sync_us_p10": pct(per, 0.1), "sync_us_p50": pct(per, 0.5),
                                             "sync_us_p90": pct(per, 0.9)})
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
