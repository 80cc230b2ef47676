"""Mask sends on the CPU (no GPU): `Node.send_output(output_id, tensor.masked(values, mask))`, bare
and under `tensor.ragged`, of numpy values through a host-only two-node dataflow — inline samples
and shared-memory ones, a bare tensor, dicts and ragged batches, masks as Python lists, bool and
uint8 arrays, an unaligned slice and a CPU torch tensor, a read-only field — arrives as the
pyarrow array of tensor.from_numpy_masked with the oracle's type info: the child keeps its N rows,
the offsets say how many are live, and `unbind()` cuts the selected rows; what the library
refuses raises and nothing is delivered."""
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


def selected(values, mask):
    keep = np.asarray(mask) != 0
    if isinstance(values, dict):
        return {k: v[keep] for k, v in values.items()}
    return values[keep]


def test_host_dataflow_delivers_masked_rows(lib):
    import torch
    out = lr.base(np.float32, (100, 6))
    det = {"bbox": out[:, :4], "conf": out[:, 4], "cls": out[:, 5]}
    big = values_of(lr.clouds(400))
    ro = np.broadcast_to(np.arange(5, dtype=np.float32), (9, 5))  # read-only: no capsule
    rng = np.random.default_rng(5)
    keep = rng.random(100) < 0.4
    wide = np.zeros(103, np.uint8)
    wide[3:] = keep * 0x80
    sent = [  # (values, mask as given, partition keyword and value or None)
        (out[:, :4], keep.tolist(), None),
        (out[:, :4], keep, None),
        (det, keep.astype(np.uint8) * 0xFF, None),
        (det, torch.from_numpy(keep), None),
        (det, wide[3:], None),                                         # any byte alignment
        (det, np.zeros(100, np.bool_), None),
        (det, np.ones(100, np.bool_), None),
        (out[::-1, 1:5], out[::-1, 4] > 300, None),
        (big, rng.random(400) < 0.5, None),                            # shared memory
        (det, keep, ("lengths", [30, 0, 70])),
        (det, keep, ("offsets", np.array([0, 100], np.int32))),
        (out[:, :4], keep, ("lengths", torch.tensor([0, 100]))),
        ({k: v[:0] for k, v in det.items()}, np.zeros(0, np.bool_), None),
        ({k: v[:0] for k, v in det.items()}, [], ("lengths", [0, 0])),
        (ro, np.arange(9) % 3 == 0, None),
        ({"same": ro, "n": np.arange(9)}, np.arange(9) > 6, ("offsets", [0, 8, 9])),
    ]

    def as_mask(m):
        m = np.asarray(m)
        return m.astype(np.bool_) if m.size == 0 else m
    wants = [tensor.from_numpy_masked(v, as_mask(m), **({p[0]: np.asarray(p[1])} if p else {}))
             for v, m, p in sent]
    assert len(pack(wants[0])[0]) < 4096 <= len(pack(wants[8])[0])
    d = InProcessDaemon(DESC)
    nodes = _start_nodes(d.shm, ["src", "dst"])
    a, b = nodes["src"], nodes["dst"]
    try:
        for k, (v, m, p) in enumerate(sent):
            t = tensor.masked(v, np.zeros(0, np.bool_) if isinstance(m, list) and not m else m)
            a.send_output("out", tensor.ragged(t, **{p[0]: p[1]}) if p else t, {"k": k})
        for k, (v, m, p) in enumerate(sent):
            ev = b.next(timeout=5)
            assert ev["type"] == "INPUT" and ev["metadata"] == {"k": k}
            want, got = wants[k], ev["value"]
            assert got.type == want.type and got.equals(want), k
            got.validate(full=True)
            assert ev["type_info"].to_json() == pack(want)[1].to_json(), k
            r = tensor.to_numpy(got)
            assert isinstance(got, pa.ListArray) and isinstance(r, tensor.Ragged), k
            n, live = len(as_mask(m)), int((as_mask(m) != 0).sum())
            assert len(got.values) == n and got.offsets.to_pylist()[-1] == live, k
            # the live rows are the selected ones, in source order
            lists = r.unbind()
            cat = {f: np.concatenate([x[f] for x in lists]) for f in lists[0]} \
                if isinstance(v, dict) else np.concatenate(lists)
            assert same_values(cat, selected(v, as_mask(m))), k
        # what the library refuses: nothing leaves
        for data, word in (
                (tensor.masked(det, keep[:99]), "mask has 99 elements, the values have 100 rows"),
                (tensor.masked(det, keep.astype(np.int32)), "is not bool or uint8"),
                (tensor.masked(det, keep.reshape(100, 1)), "mask has 2 dimensions"),
                (tensor.masked(det, np.zeros(200, np.bool_)[::2]), "the mask is dense"),
                # the partition describes the N source rows, not the K selected ones
                (tensor.ragged(tensor.masked(det, keep), lengths=[int(keep.sum())]), "100 rows"),
                (tensor.masked({"a": np.zeros((3, 2)), "b": np.zeros(4)}, [True, False, True]),
                 "field 1 `b`")):
            with pytest.raises(DoraGpuError) as e:
                a.send_output("out", data)
            assert e.value.code == -1 and word in str(e.value), str(e.value)
        with pytest.raises(TypeError):
            a.send_output("out", tensor.masked([1, 2, 3], [True, False, True]))
        with pytest.raises(TypeError) as e:
            a.send_output("out", object())
        assert "masked" in str(e.value)
        a.send_output("out", tensor.masked(det, keep), {"k": "last"})
        ev = b.next(timeout=5)  # the first thing to arrive after the refusals
        assert ev["metadata"] == {"k": "last"}
        assert ev["value"].equals(tensor.from_numpy_masked(det, keep))
    finally:
        a.close()
        b.close()
        d.join()
