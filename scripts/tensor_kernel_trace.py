"""Kernel intervals of the tensor send probe, from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --stats -d OUT -o gather -- \
        python scripts/tensor_send_probe.py --messages 20 --rounds 1 \
            --modes gather,send_raw,kernel --out OUT/probe.jsonl
    python scripts/tensor_kernel_trace.py OUT/gather_results.db profiles/tensor_send_probe_kernel_trace.jsonl

One JSON line per dispatch of the gather kernel, of the runtime's stream-write kernel (the fill
epoch of order_fill) and of the AQL pack kernels, in start order: kernel name (arguments cut),
stream and queue ids, grid, start and duration in ns.  The last line summarises the gather
kernel per grid size (one per view): count, p10 / p50 / p90 duration in us."""
import json
import sqlite3
import sys


def main(db, out):
    c = sqlite3.connect(db)
    rows = list(c.execute(
        "select name, stream_id, queue_id, grid_x, start, end - start from kernels where name like "
        "'%gather_rows_kernel%' or name like '%streamOpsWrite%' or name like 'dora_aql%' order by start"))
    by_grid = {}
    with open(out, "w") as f:
        for name, stream, queue, grid, start, dur in rows:
            short = next((k for k in ("gather_rows_kernel", "streamOpsWrite") if k in name),
                         name.split("(")[0])
            f.write(json.dumps({"kernel": short, "stream": stream, "queue": queue, "grid_x": grid,
                                "start_ns": start, "dur_ns": dur}) + "\n")
            if short == "gather_rows_kernel":
                by_grid.setdefault(grid, []).append(dur)
        summary = {}
        for grid, d in sorted(by_grid.items()):
            d.sort()
            summary[str(grid)] = {"n": len(d), "p10_us": d[len(d) // 10] / 1e3, "p50_us": d[len(d) // 2] / 1e3,
                                  "p90_us": d[(9 * len(d)) // 10] / 1e3}
        f.write(json.dumps({"gather_rows_kernel_by_grid": summary}) + "\n")
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
