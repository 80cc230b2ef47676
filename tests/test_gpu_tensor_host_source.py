"""Host tensors sent by a node with a GPU: a strided numpy view is gathered by the CPU inside the
send and then takes the paths of any host source — inline below 4096 B, the BAR fill up to 2 MiB,
the DMA above — into a device sample whose bytes and ArrowTypeInfo are the oracle's for the
nested FixedSizeList array of the view."""
import ctypes
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _nodes(df, spec):
    from dora_amd.node import Node
    out = {}

    def mk(i, d):
        out[i] = Node(i, dataflow=df.shm, device=d)
    ts = [threading.Thread(target=mk, args=(i, d)) for i, d in spec.items()]
    [t.start() for t in ts]
    [t.join(90) for t in ts]
    assert set(out) == set(spec)
    return out


def _bytes(ev, stream):
    from dora_amd._lib import call
    if not ev["on_device"]:
        return ctypes.string_at(ev["data_ptr"], ev["data_len"])
    out = ctypes.create_string_buffer(max(ev["data_len"], 1))
    call("dora_gpu_memcpy_async", out, ev["data_ptr"], ev["data_len"], stream.handle)
    stream.sync()
    return out.raw[:ev["data_len"]]


def test_device_node_sends_strided_host_tensors(launcher):
    from dora_amd import device, tensor
    from dora_amd.dataflow import Dataflow
    from oracle.pack_ref import pack
    desc = {"nodes": [
        {"id": "src", "path": "dynamic", "outputs": ["x"]},
        {"id": "dst", "path": "dynamic", "inputs": {"x": {"source": "src/x", "queue_size": 10}}},
    ]}
    rng = np.random.default_rng(7)
    views = [rng.random((5, 7), np.float32).T,                                    # 140 B: inline
             np.moveaxis(rng.integers(0, 256, (37, 53, 3), np.uint8), -1, 0),     # 5.9 KB: BAR fill
             rng.random((1100, 1024), np.float32).T,                              # 4.5 MB: DMA
             rng.integers(0, 1 << 15, (40, 60), np.int16)[::-1, ::2],             # negative stride
             rng.random((6, 1024), np.float64)]                                   # dense, 48 KB
    got = []
    s = device.Stream()
    with Dataflow(desc, launcher=launcher) as df:
        n = _nodes(df, {"src": 0, "dst": 0})
        tx, rx = n["src"], n["dst"]
        try:
            before = tx.host_paths()["bar_fills"]
            for k, x in enumerate(views):
                tx.send_output("x", x, {"k": k})
                ev = rx.next(timeout=60)
                assert ev["type"] == "INPUT" and ev["metadata"] == {"k": k}
                value = tensor.to_numpy(ev["value"].to_pyarrow() if ev["on_device"] else ev["value"])
                got.append((_bytes(ev, s), ev["type_info"].to_json(), bool(ev["on_device"]),
                            value.copy()))
                del ev, value
            bar_fills = tx.host_paths()["bar_fills"] - before
        finally:
            for k in n.values():
                k.close()
            s.close()
    for x, (raw, info, on_device, value) in zip(views, got):
        want, winfo = pack(tensor.from_numpy(np.ascontiguousarray(x)))
        where = (x.dtype.name, x.shape)
        assert raw == bytes(want) == np.ascontiguousarray(x).tobytes(), where
        assert info == winfo.to_json(), where
        assert on_device == (len(want) >= 4096), where
        assert value.shape == x.shape and np.array_equal(value, x), where
    assert bar_fills >= 1  # (the large BAR is there on an MI355X box)


def test_pinned_source_has_been_read_when_the_send_returns(launcher):
    """A tensor in pinned host memory (declared ARROW_DEVICE_ROCM_HOST, as a pinned torch tensor
    is): a DMA or kernel would read it asynchronously to the host, so the send copies it inside
    the call.  The source is overwritten as soon as each send returns; the receiver still gets
    the bytes it held before — dense above the BAR-fill limit (the DMA path), dense small, and
    strided."""
    from ctypes import byref, c_void_p

    from dora_amd import _lib, device, tensor
    from dora_amd._lib import ARROW_DEVICE_ROCM_HOST, call
    from dora_amd.dataflow import Dataflow
    from dora_amd.node import encode_parameters
    desc = {"nodes": [
        {"id": "src", "path": "dynamic", "outputs": ["x"]},
        {"id": "dst", "path": "dynamic", "inputs": {"x": {"source": "src/x", "queue_size": 10}}},
    ]}
    device.set_device(0)
    shape = (1100, 1024)                      # 4.5 MB of float32
    nbytes = shape[0] * shape[1] * 4
    p = c_void_p()
    call("dora_gpu_host_alloc", byref(p), nbytes)
    pinned = np.frombuffer((ctypes.c_uint8 * nbytes).from_address(p.value), np.float32).reshape(shape)
    rng = np.random.default_rng(11)
    got, want = [], []
    s = device.Stream()
    try:
        with Dataflow(desc, launcher=launcher) as df:
            n = _nodes(df, {"src": 0, "dst": 0})
            tx, rx = n["src"], n["dst"]
            try:
                for k, view in enumerate((pinned, pinned[:3], pinned.T, pinned[:64, ::2])):
                    pinned[...] = rng.random(shape, np.float32)
                    want.append(np.ascontiguousarray(view).tobytes())
                    t, keep = tensor._describe_array(view)
                    params = encode_parameters({"k": k})
                    _lib.check(_lib.load().dora_node_send_output_tensor(
                        tx.handle, b"x", byref(t), ARROW_DEVICE_ROCM_HOST, params, len(params), 0))
                    pinned[...] = -1.0        # the source is the caller's again
                    ev = rx.next(timeout=60)
                    assert ev["type"] == "INPUT" and ev["metadata"] == {"k": k}
                    got.append(_bytes(ev, s))
                    del ev
            finally:
                for k in n.values():
                    k.close()
    finally:
        s.close()
        del pinned
        call("dora_gpu_host_free", p)
    assert [len(g) for g in got] == [len(w) for w in want]
    assert got == want
