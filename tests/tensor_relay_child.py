"""Relay process of tests/tensor_torch_child.py: node `rly` in a process of its own, so that the
sample it receives lies in a slot of another process that hipIpcOpenMemHandle mapped here.  It
takes torch.from_dlpack of the input and sends a transposed view of it: a strided device tensor
whose memory this process never allocated.  The report says what the runtime answered for that
pointer (hipMemGetAddressRange) and whether the send went through.

    python tests/tensor_relay_child.py DATAFLOW REPORT.json H W
"""
import ctypes
import json
import os
import sys
import traceback

import torch  # before dora_amd: one HIP runtime for both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def address_range(ptr):
    """(status, offset of ptr in the allocation, its size) by hipMemGetAddressRange of the HIP
    runtime this process has loaded."""
    path = None
    with open("/proc/self/maps") as f:
        for line in f:
            p = line.rsplit(None, 1)[-1]
            if os.path.basename(p).startswith("libamdhip64"):
                path = p
                break
    hip = ctypes.CDLL(path)
    base, size = ctypes.c_void_p(), ctypes.c_size_t()
    rc = hip.hipMemGetAddressRange(ctypes.byref(base), ctypes.byref(size), ctypes.c_void_p(ptr))
    return int(rc), (ptr - (base.value or 0)) if rc == 0 else None, int(size.value)


def main(shm, report_path, h, w):
    report = {"ready": False}

    def save():
        with open(report_path + ".tmp", "w") as f:
            json.dump(report, f)
        os.replace(report_path + ".tmp", report_path)
    try:
        from dora_amd.node import Node
        torch.cuda.set_device(0)
        node = Node("rly", dataflow=shm, device=0)
        try:
            report["ready"] = True
            save()
            ev = node.next(timeout=60)
            assert ev["type"] == "INPUT" and ev["on_device"], ev["type"]
            report["ipc_opens"] = node.dataflow_counters("rly")["ipc_opens"]
            got = torch.from_dlpack(ev["value"])
            report["address_range"] = address_range(got.data_ptr())
            view = got.view(h, w).T
            try:
                node.send_output("z", view, {"k": 8})
                report["sent"] = True
            except Exception:
                report["sent"] = False
                report["send_error"] = traceback.format_exc()[-1500:]
            save()
            del view, got, ev
            while True:  # the sample stays this process's until the test has read it
                ev = node.next(timeout=60)
                if ev is None or ev["type"] != "INPUT" or ev["metadata"].get("quit"):
                    break
                del ev
        finally:
            node.close()
    except Exception:
        report["error"] = traceback.format_exc()[-1500:]
    save()


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
