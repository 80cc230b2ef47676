"""Ragged-batch sends on the CPU (no GPU): `Node.send_output(output_id, tensor.ragged(values,
lengths= / offsets=))` of numpy values through a host-only two-node dataflow — an inline sample
and shared-memory ones, a bare tensor and records, partitions as Python lists, int32 and int64
arrays and a CPU torch tensor — arrives as the pyarrow ListArray of tensor.from_numpy_ragged with
the oracle's type info; tensor.ragged_type / from_numpy_ragged / to_numpy / to_torch and
Ragged.lengths / unbind on host arrays; and what the Python layer and the plan refuse."""
import numpy as np
import pyarrow as pa
import pytest

from dora_amd import tensor
from dora_amd._lib import DoraGpuError
from oracle.pack_ref import pack
from tests import list_records as lr
from tests.test_dataflow_host import InProcessDaemon, _start_nodes

DESC = {"nodes": [
    {"id": "src", "outputs": ["out"]},
    {"id": "dst", "inputs": {"in": {"source": "src/out", "queue_size": 100}}, "outputs": []},
]}


def values_of(rec):
    return rec[0][2] if rec[0][0] is None else {name: v for name, _, v in rec}


def same_values(got, want):
    if isinstance(want, dict):
        return list(got) == list(want) and all(same_values(got[k], want[k]) for k in want)
    return got.shape == want.shape and got.dtype == want.dtype and \
        got.tobytes() == np.ascontiguousarray(want).tobytes()


def test_types_and_round_trip_on_the_host():
    d = values_of(lr.clouds(13))
    arr = tensor.from_numpy_ragged(d, lengths=[0, 6, 0, 7, 0])
    assert isinstance(arr, pa.ListArray) and len(arr) == 5
    assert arr.type == tensor.ragged_type({k: (v.dtype, v.shape) for k, v in d.items()})
    assert arr.type == pa.list_(pa.struct([("x", pa.float32()), ("y", pa.float32()),
                                           ("z", pa.float32()), ("intensity", pa.uint8())]))
    assert arr.equals(tensor.from_numpy_ragged(d, offsets=[0, 0, 6, 6, 13, 13]))
    arr.validate(full=True)
    r = tensor.to_numpy(arr)
    assert isinstance(r, tensor.Ragged) and len(r) == 5 and same_values(r.values, d)
    assert r.offsets.dtype == np.int32 and r.offsets.tolist() == [0, 0, 6, 6, 13, 13]
    assert r.lengths().tolist() == [0, 6, 0, 7, 0]
    rows = r.unbind()
    assert [len(x["x"]) for x in rows] == [0, 6, 0, 7, 0]
    assert rows[3]["intensity"].tobytes() == d["intensity"][6:13].tobytes()
    # a slice of the list: its own offsets over the whole child, as in Arrow
    part = tensor.to_numpy(arr[1:4])
    assert part.offsets.tolist() == [0, 6, 6, 13] and same_values(part.values, d)
    # a bare tensor child
    b = lr.bare(13)[0][2]
    arr = tensor.from_numpy_ragged(b, lengths=[13])
    assert arr.type == tensor.ragged_type((b.dtype, b.shape)) == pa.list_(pa.list_(pa.float32(), 4))
    r = tensor.to_numpy(arr)
    assert same_values(r.values, b) and [x.shape for x in r.unbind()] == [(13, 4)]
    t = tensor.to_torch(arr)
    assert tuple(t.values.shape) == (13, 4) and t.offsets.tolist() == [0, 13]
    assert t.lengths().tolist() == [13] and np.array_equal(t.unbind()[0].numpy(), b)
    # nulls at any level are refused, the list's own included
    with pytest.raises(TypeError):
        tensor.to_numpy(pa.array([[1], None], pa.list_(pa.int32())))
    with pytest.raises(TypeError):
        tensor.to_numpy(pa.array([[1, None]], pa.list_(pa.int32())))
    # exactly one of lengths and offsets; a partition that does not cut the rows
    with pytest.raises(TypeError):
        tensor.ragged(b)
    with pytest.raises(TypeError):
        tensor.ragged(b, lengths=[13], offsets=[0, 13])
    with pytest.raises(ValueError):
        tensor.from_numpy_ragged(b, lengths=[12])


def test_host_dataflow_delivers_ragged_batches(lib):
    import torch
    small, big, det = lr.bare(13), lr.clouds(400), lr.detector(67)
    ro = np.broadcast_to(np.arange(5, dtype=np.float32), (9, 5))  # read-only: no capsule
    sent = [  # (values, keyword, partition as given, lengths)
        (values_of(small), "lengths", [0, 6, 0, 7, 0], [0, 6, 0, 7, 0]),
        (values_of(small), "offsets", np.array([0, 13], np.int32), [13]),
        (values_of(big), "lengths", np.array([100, 0, 300], np.int64), [100, 0, 300]),
        (values_of(big), "offsets", torch.tensor([0, 0, 400, 400]), [0, 400, 0]),
        (values_of(det), "lengths", torch.tensor([60, 7], dtype=torch.int32), [60, 7]),
        (ro, "offsets", [0, 4, 9], [4, 5]),
        (values_of(lr.clouds(0)), "lengths", [0, 0, 0], [0, 0, 0]),
        (values_of(lr.bare(0)), "lengths", [], []),
    ]
    wants = [tensor.from_numpy_ragged(v, lengths=ln) for v, _, _, ln in sent]
    assert len(pack(wants[0])[0]) < 4096 <= len(pack(wants[2])[0])
    d = InProcessDaemon(DESC)
    nodes = _start_nodes(d.shm, ["src", "dst"])
    a, b = nodes["src"], nodes["dst"]
    try:
        slots = []
        for k, (v, kw, part, _) in enumerate(sent):
            a.send_output("out", tensor.ragged(v, **{kw: part}), {"k": k})
            slots.append(a.stats()["slots_created"])
        # below 4096 B the sample travels inline, in no slot; at and above it in shared memory
        assert slots[1] == 0 and slots[2] == 1
        for k, (v, _, _, ln) in enumerate(sent):
            ev = b.next(timeout=5)
            assert ev["type"] == "INPUT" and ev["metadata"] == {"k": k}
            want, got = wants[k], ev["value"]
            assert isinstance(got, pa.ListArray) and got.type == want.type and got.equals(want), k
            got.validate(full=True)
            assert ev["type_info"].to_json() == pack(want)[1].to_json(), k
            r = tensor.to_numpy(got)
            assert same_values(r.values, v) and r.lengths().tolist() == ln, k
        # refusals of the Python layer and of the plan, and the next send still arrives
        x = values_of(small)
        with pytest.raises(TypeError):
            a.send_output("out", tensor.ragged([1, 2, 3], lengths=[3]))
        with pytest.raises(TypeError) as e:
            a.send_output("out", tensor.ragged({"a": np.zeros(3), "b": [1, 2, 3]}, lengths=[3]))
        assert "`b`" in str(e.value)
        with pytest.raises(TypeError):
            a.send_output("out", tensor.ragged(x, lengths=[6.5, 6.5]))
        with pytest.raises(DoraGpuError) as e:
            a.send_output("out", tensor.ragged(x, lengths=[6, -1, 8]))
        assert e.value.code == -1 and "length 1 is -1" in str(e.value)
        with pytest.raises(DoraGpuError) as e:
            a.send_output("out", tensor.ragged(x, lengths=np.array([6, 6], np.int32)))
        assert e.value.code == -1 and "sum to 12" in str(e.value) and "13 rows" in str(e.value)
        with pytest.raises(DoraGpuError) as e:
            a.send_output("out", tensor.ragged(x, offsets=[0, 7, 6, 13]))
        assert e.value.code == -1 and "offset 2 is 6" in str(e.value)
        with pytest.raises(DoraGpuError) as e:
            a.send_output("out", tensor.ragged(x, offsets=[1, 13]))
        assert e.value.code == -1 and "offset 0 is 1" in str(e.value)
        with pytest.raises(DoraGpuError) as e:
            a.send_output("out", tensor.ragged({"a": np.zeros((3, 2)), "b": np.zeros(4)}, lengths=[3]))
        assert e.value.code == -1 and "field 1 `b`" in str(e.value)
        with pytest.raises(DoraGpuError) as e:
            a.send_output("out", tensor.ragged({"a": np.zeros(3), "m": np.zeros(3, np.bool_)},
                                               lengths=[3]))
        assert e.value.code == -4 and "field 1 `m`" in str(e.value) and "bool" in str(e.value)
        with pytest.raises(DoraGpuError) as e:
            a.send_output("out", tensor.ragged(np.zeros(3, np.bool_), lengths=[3]))
        assert e.value.code == -4 and "field" not in str(e.value) and "bool" in str(e.value)
        with pytest.raises(DoraGpuError) as e:
            a.send_output("out", tensor.ragged({f"f{k}": np.zeros(2) for k in range(9)}, lengths=[2]))
        assert e.value.code == -4
        with pytest.raises(TypeError) as e:
            a.send_output("out", object())
        assert "ragged" in str(e.value)
        a.send_output("out", tensor.ragged(x, lengths=[13]), {"k": "last"})
        ev = b.next(timeout=5)
        assert ev["metadata"] == {"k": "last"} and same_values(tensor.to_numpy(ev["value"]).values, x)
    finally:
        a.close()
        b.close()
        d.join()
