"""Probe: what sending rows selected by a bool mask in HBM costs against what a producer does
without `tensor.masked`, both of which this tree contains unchanged and both of which synchronise
with the GPU before the send:

  nonzero_take   idx = mask.nonzero().squeeze(1); send_output("s", tensor.take(fields, idx))
  index_mask     send_output("s", {name: view[mask], ..})
  masked         send_output("s", tensor.masked(fields, mask)): no synchronisation, N rows written
                 instead of K

Records, src and sink on GPU 0 of one process, each at every set fraction of `--fractions`:

  detector_25200   {bbox: out[:, :4], conf: out[:, 4], cls: out[:, 5]} of a (25200, 6) float32
  cloud_1000000    {x, y, z: columns of a (1000000, 3) float32, intensity: float32}

Modes are interleaved in `--rounds` rounds of `--messages` synchronous sends each; the time is
that of the synchronous call of one message, the yardsticks' nonzero / indexing inside the clock
(p10 / p50 / p90 us over the round; the sink drains after the clock stops).  One JSON line per
(record, fraction, mode, round) goes to `--out`.

    python scripts/tensor_mask_probe.py --out profiles/tensor_mask_probe.jsonl

Device time per launch comes from a kernel trace of the same script, a run of its own without
counters, read back with `--trace-db` (same `--messages`, `--records`, `--fractions` and `--modes`,
one round).  A 16-byte fill_kernel launch ends the warm-up and the measured block of every
(record, fraction, mode) in the trace:

    rocprofv3 --kernel-trace --stats -d OUT -o mask -- \\
        python scripts/tensor_mask_probe.py --messages 50 --rounds 1 --modes masked --out OUT/probe.jsonl
    python scripts/tensor_mask_probe.py --messages 50 --modes masked --trace-db OUT/mask_results.db \\
        --out profiles/tensor_mask_probe.jsonl --append

which adds one line per (record, fraction): p10 / p50 / p90 us per launch of mask_count_kernel,
mask_compact_kernel and gather_struct_kernel.
"""
import argparse
import json
import os
import sys
import threading
import time

RECORDS = ("detector_25200", "cloud_1000000")
MODES = ("nonzero_take", "index_mask", "masked")
FRACTIONS = "0.01,0.1,0.25,0.5,0.9"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESC = {"nodes": [
    {"id": "src", "path": "dynamic", "outputs": ["s"]},
    {"id": "dst", "path": "dynamic", "inputs": {"s": {"source": "src/s", "queue_size": 10}}},
]}


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))] / 1e3


def record(torch, name):
    """name -> (fields, N)."""
    dev = torch.device("cuda", 0)
    n = int(name.split("_")[1])
    if name.startswith("cloud"):
        p = torch.rand((n, 3), dtype=torch.float32, device=dev)
        i = torch.rand((n,), dtype=torch.float32, device=dev)
        return {"x": p[:, 0], "y": p[:, 1], "z": p[:, 2], "intensity": i}, n
    o = torch.rand((n, 6), dtype=torch.float32, device=dev)
    return {"bbox": o[:, :4], "conf": o[:, 4], "cls": o[:, 5]}, n


def trace_rows(db, plan, messages):
    """Per (record, fraction, mode) of the trace — two blocks each in the probe's own order, the
    warm-up and the measured messages, a fill_kernel launch after each — the device time per
    launch of each of the mask send's kernels."""
    import sqlite3
    c = sqlite3.connect(db)
    blocks, cur = [], []
    for name, dt in c.execute("select name, end - start from kernels order by start"):
        if "fill_kernel" in name:
            blocks.append(cur)
            cur = []
        else:
            cur.append((name, dt))
    if len(blocks) != 2 * len(plan) or cur:
        raise SystemExit(f"{len(blocks)} blocks in the trace ({len(cur)} launches left over), "
                         f"{2 * len(plan)} expected")
    rows = []
    for (name, frac, mode), b in zip(plan, blocks[1::2]):
        row = {"record": name, "fraction": frac, "mode": mode + "_kernel_trace",
               "messages": messages, "launches_per_message": len(b) / messages}
        for kern in ("mask_count_kernel", "mask_compact_kernel", "gather_struct_kernel"):
            per = [dt for nm, dt in b if kern in nm]
            if per:
                row[kern + "_us"] = {"p10": pct(per, 0.1), "p50": pct(per, 0.5), "p90": pct(per, 0.9),
                                     "launches": len(per)}
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_mask_probe.jsonl"))
    ap.add_argument("--messages", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--records", default=",".join(RECORDS))
    ap.add_argument("--fractions", default=FRACTIONS)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--trace-db", default="", help="read a rocprofv3 kernel trace of this probe "
                    "(one round) instead of running it")
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    names = [r for r in a.records.split(",") if r]
    modes = [m for m in a.modes.split(",") if m]
    fracs = [float(f) for f in a.fractions.split(",") if f]
    rows = []
    if a.trace_db:
        rows = trace_rows(a.trace_db, [(n, f, m) for n in names for f in fracs for m in modes],
                          a.messages)
    else:
        import torch  # before dora_amd: one HIP runtime for both (dora_amd/node.py)
        sys.path.insert(0, ROOT)
        from dora_amd import launcher as launcher_mod
        lch = launcher_mod.Launcher()  # before HIP is initialised here
        from dora_amd import device, tensor
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
                mark = device.DeviceBuffer(16)

                def end_of_block():
                    """A fill_kernel launch: where a block ends in a kernel trace."""
                    torch.cuda.synchronize()
                    device.fill_splitmix(mark.ptr, 16, 1)
                    torch.cuda.synchronize()

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
                    g = torch.Generator(device="cpu").manual_seed(5)
                    for name in names:
                        fields, rows_n = record(torch, name)
                        row_bytes = sum(v[:1].numel() * v.element_size() for v in fields.values())
                        for frac in fracs:
                            mask = (torch.rand(rows_n, generator=g) < frac).to(torch.device("cuda", 0))
                            k = int(mask.sum().item())
                            torch.cuda.synchronize()

                            def by_index():
                                return tensor.take(fields, mask.nonzero().squeeze(1))
                            make = {"nonzero_take": by_index,
                                    "index_mask": lambda: {f: v[mask] for f, v in fields.items()},
                                    "masked": lambda: tensor.masked(fields, mask)}
                            for rnd in range(a.rounds):
                                for mode in modes:
                                    if rnd == 0:  # warm up: slots, streams, code objects, the allocator
                                        for _ in range(a.warmup):
                                            one(make[mode])
                                        end_of_block()
                                    per = [one(make[mode]) for _ in range(a.messages)]
                                    end_of_block()
                                    rows.append({"record": name, "fraction": frac, "mode": mode,
                                                 "round": rnd, "rows": rows_n, "selected": k,
                                                 "messages": a.messages,
                                                 "sample_bytes": (rows_n if mode == "masked" else k) * row_bytes,
                                                 "sync_us_p10": pct(per, 0.1), "sync_us_p50": pct(per, 0.5),
                                                 "sync_us_p90": pct(per, 0.9)})
                                    print(json.dumps(rows[-1]), flush=True)
                    mark.free()
                finally:
                    for node in n.values():
                        node.close()
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
