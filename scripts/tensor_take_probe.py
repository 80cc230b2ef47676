"""Probe: what sending rows taken by an index in HBM costs against what a producer does without
`tensor.take`, which this tree contains unchanged: `torch.index_select` of every field into a
fresh tensor, then the struct or ragged send of the results.

Records, src and sink on GPU 0 of one process (K rows taken of N):

  detector_100              {bbox: out[:, :4], conf: out[:, 4], cls: out[:, 5]} of a (100, 6)
                            float32, K = 37
  detector_100000_sorted    the same of a (100000, 6) float32, K = 20000 distinct rows, ascending
  detector_100000_shuffled  the same rows in random order
  c3_sorted                 {x, y, z: columns of a (1000000, 3) float32, intensity: uint8},
                            K = 250000 distinct rows, ascending
  c3_shuffled               the same rows in random order

Modes, interleaved in `--rounds` rounds of `--messages` synchronous sends each:

  select_struct   send_output("s", {name: torch.index_select(view, 0, keep), ..}): the yardstick
  take_struct     send_output("s", tensor.take({name: view, ..}, keep))
  select_ragged   the yardstick under tensor.ragged(.., lengths=<int64 tensor in HBM>)
  take_ragged     send_output("s", tensor.ragged(tensor.take(..), lengths=<the same tensor>))

each as the time of the synchronous call of one message, the yardstick's index_select calls
inside the clock (p10 / p50 / p90 us over the round; the sink drains after the clock stops).  One
JSON line per (record, mode, round) goes to `--out`, with the algorithmic bytes of the mode: a take
reads K rows and K index words and writes K rows; the yardstick reads and writes the K rows twice
and reads the index once per field.

    python scripts/tensor_take_probe.py --out profiles/tensor_take_probe.jsonl

Device time comes from a kernel trace of the same script, a run of its own without counters, read
back with `--trace-db` (same `--messages`, `--records` and `--modes`, one round).  A 16-byte fill_kernel
launch ends the warm-up and the measured block of every (record, mode) in the trace:

    rocprofv3 --kernel-trace --stats -d OUT -o take -- \\
        python scripts/tensor_take_probe.py --messages 50 --rounds 1 --out OUT/probe.jsonl
    python scripts/tensor_take_probe.py --messages 50 --trace-db OUT/take_results.db \\
        --out profiles/tensor_take_probe.jsonl --append

which adds one line per (record, mode): the device time of the kernels of one message summed (a
take: its one gather_struct_kernel; the yardstick: index_select's kernels plus the send's), as a
mean and, where every message launched the same kernels, as p10 / p50 / p90, and their names.
"""
import argparse
import json
import os
import sys
import threading
import time

RECORDS = ("detector_100", "detector_100000_sorted", "detector_100000_shuffled", "c3_sorted",
           "c3_shuffled")
MODES = ("select_struct", "take_struct", "select_ragged", "take_ragged")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESC = {"nodes": [
    {"id": "src", "path": "dynamic", "outputs": ["s"]},
    {"id": "dst", "path": "dynamic", "inputs": {"s": {"source": "src/s", "queue_size": 10}}},
]}
LISTS = 8  # per-image counts of the ragged modes


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
    """name -> (fields, keep: K int64 row numbers in HBM, N)."""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(5)
    out, bases = {}, {}
    for name in names:
        kind = name.split("_sorted")[0].split("_shuffled")[0]
        if kind not in bases:
            if kind == "c3":
                n, k = 1000000, 250000
                p = torch.rand((n, 3), dtype=torch.float32, device=dev)
                i = torch.randint(0, 255, (n,), dtype=torch.uint8, device=dev)
                fields = {"x": p[:, 0], "y": p[:, 1], "z": p[:, 2], "intensity": i}
            else:
                n = int(kind.split("_")[1])
                k = 37 if n == 100 else n // 5
                o = torch.rand((n, 6), dtype=torch.float32, device=dev)
                fields = {"bbox": o[:, :4], "conf": o[:, 4], "cls": o[:, 5]}
            bases[kind] = (fields, torch.randperm(n, generator=g)[:k], n)
        fields, rows, n = bases[kind]
        keep = rows if name.endswith("_shuffled") else torch.sort(rows).values
        out[name] = (fields, keep.to(torch.int64).to(dev), n)
    return out


def algorithmic_bytes(fields, k, mode):
    row = sum(v[:1].numel() * v.element_size() for v in fields.values())
    if mode.startswith("take"):
        return {"read": k * row + k * 8, "written": k * row}
    return {"read": 2 * k * row + len(fields) * k * 8, "written": 2 * k * row}


def short(kernel):
    """A kernel's own name: no return type, namespaces, template or call arguments."""
    import re
    kernel = kernel.replace("(anonymous namespace)::", "")
    return re.split(r"[<(]", kernel)[0].split()[-1].split("::")[-1]


def trace_rows(db, plan, messages, warmup):
    """Per (record, mode) of the trace — two blocks each in the probe's own order, the warm-up and
    the measured messages, a fill_kernel launch after each — the device time of the measured
    block's kernels per message: the mean always, and p10 / p50 / p90 of the messages' sums where
    every message launched the same number of kernels."""
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
    for (name, mode), b in zip(plan, blocks[1::2]):
        row = {"record": name, "mode": mode + "_kernel_trace", "messages": messages,
               "kernels": sorted({short(nm) for nm, _ in b}),
               "kernels_per_message": len(b) / messages,
               "kernels_us_mean": sum(dt for _, dt in b) / messages / 1e3}
        gather = [dt for nm, dt in b if "gather_struct_kernel" in nm]
        if gather:
            row["gather_struct_kernel_us_p50"] = pct(gather, 0.5)
        if b and len(b) % messages == 0:
            each = len(b) // messages
            total = [sum(dt for _, dt in b[i * each:(i + 1) * each]) for i in range(messages)]
            row.update(kernels_us_p10=pct(total, 0.1), kernels_us_p50=pct(total, 0.5),
                       kernels_us_p90=pct(total, 0.9))
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_take_probe.jsonl"))
    ap.add_argument("--messages", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--records", default=",".join(RECORDS))
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--trace-db", default="", help="read a rocprofv3 kernel trace of this probe "
                    "(one round) instead of running it")
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    names = [r for r in a.records.split(",") if r]
    modes = [m for m in a.modes.split(",") if m]
    rows = []
    if a.trace_db:
        rows = trace_rows(a.trace_db, [(n, m) for n in names for m in modes], a.messages, a.warmup)
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
                    recs = records(torch, names)
                    torch.cuda.synchronize()
                    for name in names:
                        fields, keep, rows_n = recs[name]
                        k = keep.numel()
                        counts = torch.tensor(split(k, LISTS), dtype=torch.int64,
                                              device=torch.device("cuda", 0))
                        torch.cuda.synchronize()

                        def selected():
                            return {f: torch.index_select(v, 0, keep) for f, v in fields.items()}
                        make = {"select_struct": selected,
                                "take_struct": lambda: tensor.take(fields, keep),
                                "select_ragged": lambda: tensor.ragged(selected(), lengths=counts),
                                "take_ragged": lambda: tensor.ragged(tensor.take(fields, keep),
                                                                     lengths=counts)}
                        for rnd in range(a.rounds):
                            for mode in modes:
                                if rnd == 0:  # warm up: slots, streams, code objects, the allocator
                                    for _ in range(a.warmup):
                                        one(make[mode])
                                    end_of_block()
                                per = [one(make[mode]) for _ in range(a.messages)]
                                end_of_block()
                                rows.append({"record": name, "mode": mode, "round": rnd, "rows": rows_n,
                                             "taken": k, "messages": a.messages,
                                             "algorithmic_bytes": algorithmic_bytes(fields, k, mode),
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
