"""Struct-of-tensors sends on the CPU (no GPU): `Node.send_output(output_id, {name: tensor, ..})`
of numpy dicts through a host-only two-node dataflow — inline and shared-memory samples, strided,
dense and read-only fields — arrives as the pyarrow StructArray of tensor.from_numpy_struct with
the oracle's type info; tensor.struct_type / from_numpy_struct / to_numpy / to_torch on host
arrays; and what the Python layer refuses."""
import numpy as np
import pyarrow as pa
import pytest

from dora_amd import tensor
from dora_amd._lib import DoraGpuError
from oracle.pack_ref import pack
from tests import struct_records as sr
from tests.test_dataflow_host import InProcessDaemon, _start_nodes

DESC = {"nodes": [
    {"id": "src", "outputs": ["out"]},
    {"id": "dst", "inputs": {"in": {"source": "src/out", "queue_size": 100}}, "outputs": []},
]}


def as_dict(rec):
    return {name: v for name, _, v in rec}


def test_struct_type_and_round_trip_on_the_host():
    d = as_dict(sr.detector(5))
    arr = tensor.from_numpy_struct(d)
    assert isinstance(arr, pa.StructArray) and len(arr) == 5
    assert arr.type == tensor.struct_type({k: (v.dtype, v.shape) for k, v in d.items()})
    assert arr.type == pa.struct([("bbox", pa.list_(pa.float32(), 4)), ("conf", pa.float16()),
                                  ("label", pa.int64()), ("rgb", pa.list_(pa.uint8(), 3))])
    back = tensor.to_numpy(arr)
    assert list(back) == list(d)
    for k in d:
        assert back[k].shape == d[k].shape and back[k].dtype == d[k].dtype
        assert back[k].tobytes() == np.ascontiguousarray(d[k]).tobytes()
    # a slice of the struct gives the slice of every field
    part = tensor.to_numpy(arr[1:4])
    assert all(part[k].tobytes() == np.ascontiguousarray(d[k][1:4]).tobytes() for k in d)
    t = tensor.to_torch(arr)
    assert list(t) == list(d) and tuple(t["bbox"].shape) == (5, 4)
    assert np.array_equal(t["rgb"].numpy(), d["rgb"])
    # nulls at any level are refused, the struct's own included
    with pytest.raises(TypeError):
        tensor.to_numpy(pa.array([{"a": 1}, None], pa.struct([("a", pa.int32())])))
    with pytest.raises(TypeError):
        tensor.to_numpy(pa.array([{"a": 1}, {"a": None}], pa.struct([("a", pa.int32())])))
    with pytest.raises(ValueError):
        tensor.from_numpy_struct({})


def test_host_dataflow_delivers_numpy_dicts(lib):
    small, big = sr.detector(5), sr.detector(400, cls=True)
    ro = {"same": np.broadcast_to(np.arange(5, dtype=np.float32), (9, 5)),  # read-only: no capsule
          "rev": sr.negative_and_broadcast()[0][2]}
    one = {"image": np.moveaxis(sr.base(np.uint8, (7, 5, 3)), -1, 0)[None],
           "pose": np.arange(7, dtype=np.float64)[None]}  # unrelated shapes: a struct of length 1
    sent = [as_dict(small), as_dict(big), ro, one]
    assert len(pack(tensor.from_numpy_struct(sent[0]))[0]) < 4096 <= len(pack(tensor.from_numpy_struct(sent[1]))[0])
    d = InProcessDaemon(DESC)
    nodes = _start_nodes(d.shm, ["src", "dst"])
    a, b = nodes["src"], nodes["dst"]
    try:
        for k, rec in enumerate(sent):
            a.send_output("out", rec, {"k": k})
        for k, rec in enumerate(sent):
            ev = b.next(timeout=5)
            assert ev["type"] == "INPUT" and ev["metadata"] == {"k": k}
            want = tensor.from_numpy_struct(rec)
            v = ev["value"]
            assert isinstance(v, pa.StructArray) and v.type == want.type and v.equals(want), k
            assert ev["type_info"].to_json() == pack(want)[1].to_json(), k
            got = tensor.to_numpy(v)
            assert list(got) == list(rec)
            assert all(got[n].shape == rec[n].shape and
                       got[n].tobytes() == np.ascontiguousarray(rec[n]).tobytes() for n in rec), k
        # refusals of the Python layer and of the plan, and the next send still arrives
        with pytest.raises(TypeError):
            a.send_output("out", {})
        with pytest.raises(TypeError) as e:
            a.send_output("out", {"a": np.zeros(3), "b": [1, 2, 3]})
        assert "`b`" in str(e.value)
        with pytest.raises(DoraGpuError) as e:
            a.send_output("out", {"a": np.zeros((3, 2)), "b": np.zeros(4)})
        assert e.value.code == -1 and "field 1 `b`" in str(e.value)
        with pytest.raises(DoraGpuError) as e:
            a.send_output("out", {"a": np.zeros(3), "m": np.zeros(3, np.bool_)})
        assert e.value.code == -4 and "field 1 `m`" in str(e.value) and "bool" in str(e.value)
        with pytest.raises(DoraGpuError) as e:
            a.send_output("out", {f"f{k}": np.zeros(2) for k in range(9)})
        assert e.value.code == -4
        a.send_output("out", {"x": np.arange(6).reshape(2, 3).T}, {"k": "last"})
        ev = b.next(timeout=5)
        assert ev["metadata"] == {"k": "last"}
        assert np.array_equal(tensor.to_numpy(ev["value"])["x"], np.arange(6).reshape(2, 3).T)
    finally:
        a.close()
        b.close()
        d.join()
