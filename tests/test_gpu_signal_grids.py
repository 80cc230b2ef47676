"""The in-kernel fill signal at every shape its poll loop distinguishes (include/
dora_gpu_device.h dora_fill_wait_all, called by pack_device.h signal_fill).

Asynchronous device-bytes sends outside the command processor's signalling window keep the
in-kernel signal (aql.cpp aql_pack): one workgroup (nothing to poll), two, 128 (fewer done words
than polling lanes) and the 1024-workgroup cap (four done words per lane, workgroups striding
over the chunks, a ragged tail).  Each must arrive byte-exact through a single-segment AQL kernel
with no help from the command processor.  A struct of nine children has more segments than an
AQL pack takes and goes through the HIP-launched signalling pack.
"""
import ctypes
import threading

import pytest

pytestmark = pytest.mark.gpu

# (bytes, workgroups): 8 KiB chunks, kSignalGrid = 1024
SIZES = [(4096, 1), (8192 + 16, 2), ((1 << 20) - 16, 128), ((33 << 20) + 5, 1024)]


def _nodes(df, spec):
    from dora_amd.node import Node
    out = {}

    def mk(i, dev):
        out[i] = Node(i, dataflow=df.shm, device=dev)
    ts = [threading.Thread(target=mk, args=(i, d)) for i, d in spec.items()]
    [t.start() for t in ts]
    [t.join(90) for t in ts]
    assert set(out) == set(spec)
    return out


def _single_segment_dispatches():
    from dora_amd import device
    c = device.aql_dispatch_counts(0)
    return c.get("dora_aql_pack1_u4", 0) + c.get("dora_aql_pack1c_u4", 0)


def test_in_kernel_signal_at_every_grid_shape(launcher):
    import numpy as np
    import pyarrow as pa
    from dora_amd import device
    from dora_amd._lib import call
    from dora_amd.dataflow import Dataflow
    from dora_amd.device import DeviceArray, DeviceBuffer
    from oracle.checksum_ref import csum64, splitmix_bytes
    from oracle.pack_ref import pack, sample_regions
    desc = {"nodes": [
        {"id": "src", "path": "dynamic", "outputs": ["x"]},
        {"id": "dst", "path": "dynamic", "inputs": {"x": {"source": "src/x", "queue_size": 4}}},
    ]}
    s = device.Stream()
    buf = DeviceBuffer(max(z for z, _ in SIZES))
    with Dataflow(desc, launcher=launcher) as df:
        n = _nodes(df, {"src": 0, "dst": 0})
        tx, rx = n["src"], n["dst"]
        for k, (z, _) in enumerate(SIZES):
            seed = 0x516A00 + k
            device.fill_splitmix(buf.ptr, z, seed, s)
            s.sync()
            cp0, one0 = device.aql_cp_signalled(0), _single_segment_dispatches()
            tx.send_output_device_bytes("x", buf.ptr, z, {"k": k}, asynchronous=True)
            tx.sync()  # the next size rewrites the source
            assert device.aql_cp_signalled(0) == cp0, z
            assert _single_segment_dispatches() - one0 == 1, z
            ev = rx.next(timeout=60)
            assert ev["metadata"] == {"k": k} and ev["data_len"] == z
            # above 8 MiB the oracle's generator is slow on the CPU: the source's own checksum
            want = (csum64(splitmix_bytes(z, seed)) if z <= (8 << 20)
                    else device.csum64(buf.ptr, z, s))
            assert device.csum64(ev["data_ptr"], z, s) == want, z
            del ev
        # nine segments: more than an AQL pack's eight, so hipLaunchKernel of pack_kernel<4, 2>
        rng = np.random.default_rng(9)
        arr = pa.StructArray.from_arrays(
            [pa.array(rng.integers(-2**31, 2**31, 1000, dtype=np.int64).astype(np.int32))
             for _ in range(9)], names=[f"c{i}" for i in range(9)])
        want, info = pack(arr)
        hip0 = tx.fill_paths()["hip"]
        with DeviceArray.from_pyarrow(arr) as da:
            tx.send_output("x", da, {"k": "struct"})
        assert tx.fill_paths()["hip"] - hip0 == 1
        ev = rx.next(timeout=60)
        assert ev["metadata"] == {"k": "struct"} and ev["on_device"]
        assert ev["type_info"].to_json() == info.to_json()
        host = ctypes.create_string_buffer(ev["data_len"])
        call("dora_gpu_memcpy_async", host, ev["data_ptr"], ev["data_len"], s.handle)
        s.sync()
        got = host.raw[:ev["data_len"]]
        assert len(got) >= len(want)
        assert sample_regions(got, ev["type_info"]) == sample_regions(want, info)
        del ev
        tx.close()
        rx.close()
        df.wait(60)
    buf.free()
    s.close()
