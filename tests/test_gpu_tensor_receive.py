"""Tensor messages on a device receiver: a host numpy tensor sent through the host path arrives
as a nested FixedSizeList DeviceArray, which `torch.from_dlpack` and `tensor.to_torch` export
zero-copy as one kDLROCM tensor of its shape (data pointer inside the slot); nulls are refused;
the input's token returns only after the tensor is dropped."""
import gc
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DESC = {"nodes": [
    {"id": "src", "path": "dynamic", "outputs": ["x"]},
    {"id": "dst", "path": "dynamic", "inputs": {"x": {"source": "src/x", "queue_size": 10}}},
]}


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


def test_device_receiver_exports_tensor_messages_zero_copy(launcher):
    # (torch comes into this process after the library: with torch's bundled HIP runtime the
    # process then holds two.  Receiving works all the same, since a raw device address is valid
    # for kernels of either; only sending a device tensor needs one runtime)
    import torch
    from dora_amd import tensor
    from dora_amd.dataflow import Dataflow
    rng = np.random.default_rng(3)
    sent = [rng.random((33, 65), np.float32).T,                                # 2-D, strided source
            np.moveaxis(rng.integers(0, 256, (37, 53, 3), np.uint8), -1, 0),   # 3-D
            rng.integers(-99, 99, (4, 3, 5, 40), np.int16),                    # 4-D, dense
            rng.random((2000,), np.float64)]                                   # 1-D: the flat array
    with Dataflow(DESC, launcher=launcher) as df:
        n = _nodes(df, {"src": 0, "dst": 0})
        tx, rx = n["src"], n["dst"]
        try:
            for k, x in enumerate(sent):
                tx.send_output("x", x, {"k": k})
                ev = rx.next(timeout=60)
                assert ev["type"] == "INPUT" and ev["metadata"] == {"k": k} and ev["on_device"]
                for t in (torch.from_dlpack(ev["value"]), tensor.to_torch(ev["value"])):
                    assert t.device.type == "cuda" and tuple(t.shape) == x.shape
                    assert t.is_contiguous() and str(t.dtype) == "torch." + x.dtype.name
                    assert ev["data_ptr"] <= t.data_ptr() < ev["data_ptr"] + max(ev["data_len"], 1)
                    assert t.data_ptr() == ev["data_ptr"]  # (a tensor's values start its sample)
                    assert np.array_equal(t.cpu().numpy(), x)
                    del t
                del ev
            # the token of an input returns only after the tensor over it is dropped
            def settled():
                tx.send_output("x", b"", {"k": "tick"})  # a send handles returned tokens
                assert rx.next(timeout=60)["metadata"] == {"k": "tick"}
                return tx.stats()["in_flight"]

            def settle_to(level):
                deadline = time.monotonic() + 10
                while (now := settled()) > level and time.monotonic() < deadline:
                    pass
                return now
            gc.collect()
            assert settle_to(0) == 0  # every earlier input was dropped
            tx.send_output("x", sent[0], {"k": "held"})
            ev = rx.next(timeout=60)
            t = tensor.to_torch(ev["value"])
            del ev
            gc.collect()
            for _ in range(5):
                held = settled()
            assert held == 1, held
            assert np.array_equal(t.cpu().numpy(), sent[0])
            del t
            gc.collect()
            assert settle_to(0) == 0
        finally:
            for k in n.values():
                k.close()


def test_nulls_are_refused():
    import pyarrow as pa
    from dora_amd import tensor
    from dora_amd.device import DeviceArray
    ok = pa.array([[1, 2], [3, 4], [5, 6]], pa.list_(pa.int32(), 2))
    for arr in (pa.array([[1, 2], None, [5, 6]], pa.list_(pa.int32(), 2)),
                pa.array([[1, None], [3, 4]], pa.list_(pa.int32(), 2)),
                pa.array([[[1, 2]], None], pa.list_(pa.list_(pa.int32(), 2), 1))):
        with DeviceArray.from_pyarrow(arr) as da:
            with pytest.raises(TypeError):
                da.__dlpack__()
    # a slice of a tensor message exports the values of its own rows
    import torch
    with DeviceArray.from_pyarrow(ok.slice(1, 2)) as da:
        t = tensor.to_torch(da)
        assert tuple(t.shape) == (2, 2) and t.cpu().tolist() == [[3, 4], [5, 6]]
        del t
    del torch
