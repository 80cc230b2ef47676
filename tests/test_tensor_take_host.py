"""Take sends on the CPU (no GPU): `Node.send_output(output_id, tensor.take(values, index))`, bare
and under `tensor.ragged`, of numpy values through a host-only two-node dataflow — inline samples
and shared-memory ones, a bare tensor, dicts and ragged batches, indices as Python lists, int32
and int64 arrays and a CPU torch tensor, a read-only field — arrives as the pyarrow array of
tensor.from_numpy_take with the oracle's type info, and tensor.to_numpy gives back
`values[index]`; a host index with a word that is no row raises and nothing is delivered."""
import numpy as np
import pyarrow as pa
import pytest

from dora_amd import tensor
from dora_amd._lib import DoraGpuError
from oracle.pack_ref import pack
from tests import list_records as lr
from tests.test_dataflow_host import InProcessDaemon, _start_nodes
from tests.test_tensor_list_host import same_values, values_of

DESC = {"nodes": [
    {"id": "src", "outputs": ["out"]},
    {"id": "dst", "inputs": {"in": {"source": "src/out", "queue_size": 100}}, "outputs": []},
]}


def indexed(values, index):
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    if isinstance(values, dict):
        return {k: v[index] for k, v in values.items()}
    return values[index]


def test_host_dataflow_delivers_takes(lib):
    import torch
    out = lr.base(np.float32, (100, 6))
    det = {"bbox": out[:, :4], "conf": out[:, 4], "cls": out[:, 5]}
    big = values_of(lr.clouds(400))
    ro = np.broadcast_to(np.arange(5, dtype=np.float32), (9, 5))  # read-only: no capsule
    rng = np.random.default_rng(5)
    keep = rng.integers(0, 100, 37)
    sent = [  # (values, index as given, partition keyword and value or None)
        (out[:, :4], keep.tolist(), None),
        (out[:, :4], keep.astype(np.int32), None),
        (det, keep, None),
        (det, torch.from_numpy(keep), None),
        (det, [], None),
        (out[::-1, 1:5], [99, 0, 0, 50], None),
        (big, rng.integers(0, 400, 1000), None),                       # K > N, shared memory
        (det, keep, ("lengths", [30, 0, 7])),
        (det, keep.astype(np.int32), ("offsets", np.array([0, 37], np.int32))),
        (out[:, :4], keep, ("lengths", torch.tensor([0, 37]))),
        (det, [], ("lengths", [0, 0])),
        (ro, [8, 8, 0], None),
        ({"same": ro, "n": np.arange(9)}, np.array([3, 1]), ("offsets", [0, 1, 2])),
    ]
    wants = [tensor.from_numpy_take(v, np.asarray(ix, dtype=np.int64) if len(ix) == 0 else np.asarray(ix),
                                    **({p[0]: p[1]} if p else {})) for v, ix, p in sent]
    assert len(pack(wants[0])[0]) < 4096 <= len(pack(wants[6])[0])
    d = InProcessDaemon(DESC)
    nodes = _start_nodes(d.shm, ["src", "dst"])
    a, b = nodes["src"], nodes["dst"]
    try:
        for k, (v, ix, p) in enumerate(sent):
            t = tensor.take(v, ix)
            a.send_output("out", tensor.ragged(t, **{p[0]: p[1]}) if p else t, {"k": k})
        for k, (v, ix, p) in enumerate(sent):
            ev = b.next(timeout=5)
            assert ev["type"] == "INPUT" and ev["metadata"] == {"k": k}
            want, got = wants[k], ev["value"]
            assert got.type == want.type and got.equals(want), k
            got.validate(full=True)
            assert ev["type_info"].to_json() == pack(want)[1].to_json(), k
            r = tensor.to_numpy(got)
            if p:
                assert isinstance(got, pa.ListArray) and isinstance(r, tensor.Ragged), k
                r = r.values
            assert same_values(r, indexed(v, ix)), k
        # a word that is no row: the send raises, naming it, and nothing leaves
        for bad, word in (([0, 5, -1], "word 2 is -1"), ([100], "word 0 is 100"),
                          (np.array([3, 1 << 40]), f"word 1 is {1 << 40}")):
            for data in (tensor.take(det, bad), tensor.take(out[:, :4], bad),
                         tensor.ragged(tensor.take(det, bad), lengths=[len(bad)])):
                with pytest.raises(DoraGpuError) as e:
                    a.send_output("out", data)
                assert e.value.code == -1 and word in str(e.value) and "100 rows" in str(e.value)
        # the partition describes the K taken rows, not the N source rows
        with pytest.raises(DoraGpuError) as e:
            a.send_output("out", tensor.ragged(tensor.take(det, [1, 2, 3]), lengths=[100]))
        assert e.value.code == -1 and "3 rows" in str(e.value)
        # refusals of the Python layer
        with pytest.raises(TypeError):
            a.send_output("out", tensor.take(det, [0.5]))
        with pytest.raises(TypeError):
            a.send_output("out", tensor.take([1, 2, 3], [0]))
        with pytest.raises(TypeError):
            tensor.take(tensor.take(det, [0]), [0])
        with pytest.raises(DoraGpuError) as e:
            a.send_output("out", tensor.take({"a": np.zeros((3, 2)), "b": np.zeros(4)}, [0]))
        assert e.value.code == -1 and "field 1 `b`" in str(e.value)
        with pytest.raises(TypeError) as e:
            a.send_output("out", object())
        assert "take" in str(e.value)
        a.send_output("out", tensor.take(det, [99]), {"k": "last"})
        ev = b.next(timeout=5)  # the first thing to arrive after the refusals
        assert ev["metadata"] == {"k": "last"}
        assert same_values(tensor.to_numpy(ev["value"]), indexed(det, [99]))
    finally:
        a.close()
        b.close()
        d.join()
