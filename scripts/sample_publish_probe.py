#!/usr/bin/env python3
"""In-place samples, stream-ordered against self-published, interleaved on one box.

The native benchmark node (dora-gpu-bench-source -> dora-gpu-bench-sink, one GPU) sends through
the reference benchmark's own API, allocate_data_sample + a kernel that writes the slot +
send_output_sample, with DORA_BENCH_SAMPLE_PATH=1 (the send orders the fill flag after the node
stream with hipStreamWriteValue64) and =2 (dora_sample_fill_ticket: the kernel publishes the
sample itself, no stream operation of the send), at 4096 B, 4 MiB and 40.96 MB, the two paths
alternating within every round.

    python scripts/sample_publish_probe.py [--rounds 3] [--out profiles/sample_publish_probe.jsonl]

Every dataflow is a step of its own: a child process under `timeout`, and the script stops at
the first step that does not exit 0.  One JSON line per step: µs per message (throughput
mode), latency p50, checksums verified, samples by ordering.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [4096, 4 << 20, 40960000]
PATHS = {1: "stream_ordered", 2: "self_published"}


def one(size, path, gpu):
    """One dataflow: the source with DORA_BENCH_SAMPLE_PATH=`path` at `size`."""
    import bench
    from dora_amd.dataflow import Dataflow
    n = bench.native_ladder_msgs(size)
    tmp = tempfile.mkdtemp(prefix="dora-publish-probe-")
    desc = bench.c4_descriptor(2, tmp, "kernel", tp_n=n, gpu=lambda g: gpu)
    desc["nodes"][0]["env"].update({
        "DORA_BENCH_TP_SIZE": str(size), "DORA_BENCH_LAT_SIZES": str(size),
        "DORA_BENCH_LAT_N": "30", "DORA_BENCH_LAT_GAP_US": "1000",
        "DORA_BENCH_SAMPLE_PATH": str(path)})
    df = Dataflow(desc).start()
    try:
        codes = df.wait(120)
    finally:
        df.stop()
    r = bench._load(os.path.join(tmp, "source.json")) or {}
    sk = bench._load(os.path.join(tmp, "sink1.json")) or {}
    gbps = r.get("tp_delivered_GBps")
    dropped = sk.get("dropped_inputs", 0) or 0
    if gbps and dropped:  # only delivered messages count (run_native_ladder, bench.py)
        gbps = gbps * (n - min(dropped, n - 1)) / n
    lat = [x for x in sk.get("series", []) if x.get("input") == "latency"]
    rec = {"size": size, "path": PATHS[path], "msgs": n,
           "us_per_msg": round(size / (gbps * 1e3), 3) if gbps else None,
           "lat_p50_us": lat[0]["p50_us"] if lat else None,
           "lat_p50_incl_write_us": lat[0]["full_p50_us"] if lat else None,
           "verified": sum(x.get("verified", 0) for x in sk.get("series", [])),
           "mismatches": sum(x.get("mismatches", 0) for x in sk.get("series", [])),
           "sink_dropped": dropped, "send_phase_us": r.get("send_phase_us"),
           "samples_stream_ordered": r.get("samples_stream_ordered"),
           "samples_self_published": r.get("samples_self_published"),
           "ok": r.get("ok"), "exit_codes": codes}
    print(json.dumps(rec), flush=True)
    good = r.get("ok") and not r.get("errors") and not rec["mismatches"] and \
        all(c == 0 for c in codes.values())
    return 0 if good else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_publish_probe.jsonl"))
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds per dataflow")
    ap.add_argument("--one", nargs=2, type=int, metavar=("SIZE", "PATH"),
                    help="run one step in this process (what the steps' child processes do)")
    a = ap.parse_args()
    if a.one:
        sys.exit(one(a.one[0], a.one[1], a.gpu))
    if a.rounds < 3:
        ap.error("at least three rounds")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for rnd in range(a.rounds):
            for size in SIZES:
                # alternate which path goes first, so neither always runs on the warmer box
                for path in ((1, 2) if rnd % 2 == 0 else (2, 1)):
                    p = subprocess.run(
                        ["timeout", "-k", "10", str(a.step_timeout), sys.executable,
                         os.path.abspath(__file__), "--gpu", str(a.gpu), "--one", str(size),
                         str(path)], capture_output=True, text=True)
                    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
                    rec = json.loads(lines[-1]) if lines else {"size": size, "path": PATHS[path]}
                    rec["round"] = rnd
                    rec["status"] = p.returncode
                    f.write(json.dumps(rec) + "\n")
                    f.flush()
                    print(json.dumps(rec), flush=True)
                    if p.returncode != 0:
                        sys.stderr.write(p.stderr[-4000:])
                        sys.exit(f"step size={size} path={path} exited {p.returncode}: stopping")


if __name__ == "__main__":
    main()
