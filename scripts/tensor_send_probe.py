"""Probe: what sending a strided torch tensor in HBM costs, and where the time goes.

For each view — HWC->CHW of a 1080x1920x3 uint8 frame, .T of a 1100x1024 float32, a crop of a
4096x4096 uint8, NCHW->NHWC of an 8x64x112x112 float16 — src and sink on GPU 0 of one process,
in interleaved rounds of `--messages`:

  gather       node.send_output(view): DLPack handshake on the node stream + the gather send
  send_raw     dora_node_send_output_tensor over view.data_ptr() after a device synchronise: the
               same gather send without dora_node_stream() and without the DLPack event wait
  kernel       dora_gpu_pack of the view's plan on a plain stream + stream synchronise: the
               bounds check and the gather kernel alone, no node; also N launches and one
               synchronise (`async_us_per_msg`: the kernel's own rate)
  contiguous   c = view.contiguous(); torch.cuda.current_stream().synchronize();
               node.send_output_device_bytes(c.data_ptr(), nbytes): the two-step path of a tree
               without device tensors (run this mode in that tree with the same script)
  hipmemcpy    hipMemcpyAsync (dora_gpu_memcpy_async) of the same byte count, device to device,
               + stream synchronise: the box's own copy, the ceiling

each as the synchronous call's time (p10 / p50 / p90 us over the round) and as the per-message
time of the round issued asynchronously (`sync()` every 8 messages).  One JSON line per
(view, mode, round) goes to `--out`, tagged `--tree`.

    python scripts/tensor_send_probe.py --out profiles/tensor_send_probe.jsonl
    python scripts/tensor_send_probe.py --modes contiguous,hipmemcpy --tree parent --out ...
    python scripts/tensor_send_probe.py --modes send_raw,kernel --gather-kernel tile --out ...

The kernels' own device times come from a kernel trace of the same script:
scripts/tensor_kernel_trace.py.
"""
import argparse
import json
import os
import sys
import threading
import time
from ctypes import byref, c_void_p

import torch  # before dora_amd: one HIP runtime for both (dora_amd/node.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dora_amd import launcher as launcher_mod  # noqa: E402

DESC = {"nodes": [
    {"id": "src", "path": "dynamic", "outputs": ["x"]},
    {"id": "dst", "path": "dynamic", "inputs": {"x": {"source": "src/x", "queue_size": 10}}},
]}
MODES = ("gather", "send_raw", "kernel", "contiguous", "hipmemcpy")


def views():
    dev = torch.device("cuda", 0)
    frame = torch.randint(0, 255, (1080, 1920, 3), dtype=torch.uint8, device=dev)
    mat = torch.rand((1100, 1024), dtype=torch.float32, device=dev)
    big = torch.randint(0, 255, (4096, 4096), dtype=torch.uint8, device=dev)
    act = torch.rand((8, 64, 112, 112), device=dev).to(torch.float16)
    out = {"hwc_to_chw_u8_1080x1920x3": frame.permute(2, 0, 1), "T_f32_1100x1024": mat.T,
           "crop_u8_4096x4096": big[100:3900, 37:3001], "nchw_to_nhwc_f16_8x64x112x112": act.permute(0, 2, 3, 1)}
    # the selection's other edges: element sizes 1 and 8, short contiguous extents
    out["T_f64_1100x512"] = torch.rand((1100, 512), dtype=torch.float64, device=dev).T
    out["T_u8_2200x2048"] = big[:2200, :2048].T
    out["T_f32_70400x16"] = torch.rand((70400, 16), dtype=torch.float32, device=dev).T
    out["T_f32_35200x32"] = torch.rand((35200, 32), dtype=torch.float32, device=dev).T
    out["T_f16_1100x1024"] = mat.to(torch.float16).T
    out["nchw_to_nhwc_f32_4x64x112x112"] = torch.rand((4, 64, 112, 112), device=dev).permute(0, 2, 3, 1)
    return out


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))] / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_send_probe.jsonl"))
    ap.add_argument("--messages", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--tree", default="this")
    ap.add_argument("--views", default="", help="comma-separated view names (default: all)")
    ap.add_argument("--gather-kernel", choices=("auto", "rows", "tile"), default="auto",
                    help="force gather_rows_kernel / gather_tile_kernel (where it applies) through "
                         "the testing library: the keep-or-delete comparison of DESIGN §4")
    a = ap.parse_args()
    modes = [m for m in a.modes.split(",") if m]
    lch = launcher_mod.Launcher()  # before HIP is initialised here
    from dora_amd import _lib, device, tensor
    from dora_amd._lib import ARROW_DEVICE_ROCM, call
    from dora_amd.dataflow import Dataflow
    from dora_amd.node import Node
    torch.cuda.set_device(0)
    if a.gather_kernel != "auto":
        call("dora_gpu_test_gather_kernel", {"rows": 1, "tile": 2}[a.gather_kernel])
    rows = []
    try:
        with Dataflow(DESC, launcher=lch) as df:
            n = {}
            ts = [threading.Thread(target=lambda i=i: n.__setitem__(i, Node(i, dataflow=df.shm, device=0)))
                  for i in ("src", "dst")]
            [t.start() for t in ts]
            [t.join(90) for t in ts]
            tx, rx = n["src"], n["dst"]
            plain = device.Stream()
            lib = _lib.load()

            def drain():
                ev = rx.next(timeout=60)
                assert ev["type"] == "INPUT"
                del ev

            def describe(v):
                dt = torch.empty(0, dtype=v.dtype).numpy().dtype
                return tensor._describe(v.data_ptr(), tuple(v.shape), list(v.stride()), dt)

            def send(mode, v, keep, asynchronous):
                """One message of `mode`; True if the sink has something to drain."""
                flags = 1 if asynchronous else 0
                if mode == "gather":
                    tx.send_output("x", v, asynchronous=asynchronous)
                    keep.append(None)
                elif mode == "send_raw":
                    d, k = describe(v)
                    _lib.check(lib.dora_node_send_output_tensor(tx.handle, b"x", byref(d),
                                                                ARROW_DEVICE_ROCM, b"", 0, flags))
                    keep.append(k)
                elif mode == "contiguous":
                    c = v.contiguous()
                    torch.cuda.current_stream().synchronize()
                    tx.send_output_device_bytes("x", c.data_ptr(), c.numel() * c.element_size(),
                                                asynchronous=asynchronous)
                    keep.append(c)  # the pack reads it until sync()
                return True

            try:
                for name, v in views().items():
                    if a.views and name not in a.views.split(","):
                        continue
                    nbytes = v.numel() * v.element_size()
                    src_buf, dst_buf = device.DeviceBuffer(nbytes), device.DeviceBuffer(nbytes)
                    plan = None
                    if "kernel" in modes:
                        d, dkeep = describe(v)
                        h = c_void_p()
                        call("dora_gpu_plan_tensor", byref(d), ARROW_DEVICE_ROCM, byref(h))
                        plan = h.value
                    torch.cuda.synchronize()
                    for mode in modes:  # warm up: slots, streams, allocator
                        if mode in ("gather", "send_raw", "contiguous"):
                            for _ in range(10):
                                send(mode, v, [], False)
                                drain()
                    for rnd in range(a.rounds):
                        for mode in modes:
                            per = []
                            if mode in ("kernel", "hipmemcpy"):
                                def one():
                                    if mode == "kernel":
                                        call("dora_gpu_pack", plan, dst_buf.ptr, nbytes, plain.handle)
                                    else:
                                        call("dora_gpu_memcpy_async", dst_buf.ptr, src_buf.ptr, nbytes,
                                             plain.handle)
                                for _ in range(a.messages):
                                    t0 = time.perf_counter_ns()
                                    one()
                                    plain.sync()
                                    per.append(time.perf_counter_ns() - t0)
                                t0 = time.perf_counter_ns()
                                for _ in range(a.messages):
                                    one()
                                plain.sync()
                                rate = (time.perf_counter_ns() - t0) / a.messages
                            else:
                                for _ in range(a.messages):
                                    t0 = time.perf_counter_ns()
                                    send(mode, v, [], False)
                                    per.append(time.perf_counter_ns() - t0)
                                    drain()
                                keep = []
                                t0 = time.perf_counter_ns()
                                for i in range(a.messages):
                                    send(mode, v, keep, True)
                                    drain()
                                    if len(keep) >= 8:
                                        tx.sync()
                                        keep.clear()
                                tx.sync()
                                rate = (time.perf_counter_ns() - t0) / a.messages
                                keep.clear()
                            rows.append({"tree": a.tree, "gather_kernel": a.gather_kernel, "view": name, "mode": mode, "round": rnd,
                                         "bytes": nbytes, "messages": a.messages,
                                         "sync_us_p10": pct(per, 0.1), "sync_us_p50": pct(per, 0.5),
                                         "sync_us_p90": pct(per, 0.9), "async_us_per_msg": rate / 1e3,
                                         "async_GBps_2S": 2 * nbytes / rate})
                            print(json.dumps(rows[-1]), flush=True)
                    if plan:
                        lib.dora_gpu_plan_free(plan)
                    src_buf.free()
                    dst_buf.free()
            finally:
                plain.close()
                for k in n.values():
                    k.close()
    finally:
        lch.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
