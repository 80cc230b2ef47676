"""Model-input sends on the CPU (no GPU): `Node.send_output(output_id, tensor.resize(x, size,
scale=.., bias=.., axis=.., fit="letterbox", ..))` and `tensor.crops(.., scale=.., bias=..,
axis=..)`, bare and as fields of a dict next to plain fields, of numpy and CPU torch values
through a host-only two-node dataflow (daemon, receiving node over shared memory) arrive as the
pyarrow array of `tensor.from_numpy_resize` / `from_numpy_crops` with the oracle's type info, bit
for bit but for the payload of a NaN: every case of tests/prep_records.py, read-only values and
tables given as lists included.  What a send refuses raises, nothing leaves, and the next good
message is the first to arrive."""
import numpy as np
import pyarrow as pa
import pytest

from dora_amd import tensor
from dora_amd._lib import DoraGpuError
from oracle.pack_ref import pack
from tests import cast_records as cr
from tests import prep_records as pr
from tests.test_dataflow_host import InProcessDaemon, _start_nodes
from tests.test_tensor_cast_host import DESC
from tests.test_tensor_resize_host import as_values, same_arrays


oracle = pr.oracle


def sent_as(v, c):
    """What a producer sends of view `v` under op `c`."""
    kw = pr.statement_kwargs(c)
    x = as_values(c["src"], v)
    if "boxes" in c:
        return tensor.crops(x, c["boxes"], c["size"], axes=c["axes"], mode=c["mode"], dtype=c["dst"], **kw)
    return tensor.resize(x, c["size"], axes=c["axes"], mode=c["mode"], dtype=c["dst"], **kw)


def message(rec):
    """(what is sent, the array it must arrive as) of a record of tests/prep_records.py."""
    send, cols = {}, []
    for name, _, v, c in rec:
        send[name] = v if c is None else sent_as(v, c)
        cols.append(tensor.from_numpy(pr.want(v, c)))
    if len(rec) == 1 and rec[0][0] is None:
        return send[None], cols[0]
    return send, pa.StructArray.from_arrays(cols, names=[r[0] for r in rec])


def test_host_dataflow_delivers_model_inputs(lib):
    import torch
    sent = [message(rec) for _, rec, _ in pr.cases()]
    frame = cr.source("uint8", (12, 16, 3), seed=3)
    ro = np.broadcast_to(np.arange(15, dtype=np.uint8).reshape(5, 3), (6, 5, 3))  # read-only: no capsule
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    s = [1 / (255 * d) for d in std]
    b = [-m / d for m, d in zip(mean, std)]
    kw = dict(mode="bilinear", dtype="float16", scale=s, bias=b, axis=0, fill=114.0)
    inner, lead = tensor.letterbox((12, 16), (8, 8))
    sent += [
        # a CPU torch frame through permute(2, 0, 1), letterboxed, tables as lists
        (tensor.resize(torch.from_numpy(frame).permute(2, 0, 1), (8, 8), fit="letterbox", **kw),
         tensor.from_numpy_resize(frame.transpose(2, 0, 1), (8, 8), inner=inner, lead=lead, **kw)),
        # tables as a torch tensor and a numpy array of float64
        (tensor.resize(frame, (8, 8), axes=(0, 1), scale=torch.tensor(s), bias=np.array(b), axis=-1, anchor="start",
                       fit="letterbox"),
         tensor.from_numpy_resize(frame, (8, 8), axes=(0, 1), scale=s, bias=b, axis=2, inner=inner, lead=(0, 0))),
        (tensor.resize(ro, (3, 9), axes=(0, 1), mode="bilinear", bias=0.5, dtype="float32"),
         tensor.from_numpy_resize(ro, (3, 9), axes=(0, 1), mode="bilinear", bias=0.5, dtype="float32")),
        ({"crop": tensor.crops(ro, [[0, 0, 3, 3], [9, 9, 9, 9]], (2, 2), axes=(0, 1), scale=s, bias=b, axis=2,
                               dtype="float16"), "id": np.arange(2)},
         pa.StructArray.from_arrays(
             [tensor.from_numpy_crops(ro, [[0, 0, 3, 3], [9, 9, 9, 9]], (2, 2), axes=(0, 1), scale=s, bias=b,
                                      axis=2, dtype="float16"), tensor.from_numpy(np.arange(2))],
             names=["crop", "id"])),
    ]
    d = InProcessDaemon(DESC)
    nodes = _start_nodes(d.shm, ["src", "dst"])
    a, bnode = nodes["src"], nodes["dst"]
    try:
        for k, (data, want) in enumerate(sent):
            a.send_output("out", data, {"k": k})
            ev = bnode.next(timeout=5)
            assert ev["type"] == "INPUT" and ev["metadata"] == {"k": k}
            got = ev["value"]
            got.validate(full=True)
            same_arrays(got, want, k)
            assert ev["type_info"].to_json() == pack(want)[1].to_json(), k
        # refusals inside the send: nothing leaves
        x = cr.source("float32", (4, 3, 5))
        for data, code, word in (
                (tensor.resize(x, (2, 2), scale=[1, 2, 3], axis=1), -1, "resized axes"),
                (tensor.resize(x, (2, 2), scale=[1, 2, 3], axis=0), -1, "3 elements"),
                (tensor.resize(x, (2, 2), scale=[1, 2, 3, np.inf], axis=0), -1, "not finite"),
                (tensor.resize(x, (2, 2), bias=float("nan")), -1, "not finite"),
                (tensor.resize(x, (2, 2), inner=(3, 1)), -1, "inner[0] 3"),
                (tensor.resize(x, (2, 2), inner=(1, 1), lead=(2, 0)), -1, "lead[0] 2"),
                (tensor.resize(x, (2, 2), inner=(1, 1), fill=float("inf")), -1, "fill"),
                ({"a": x, "b": tensor.resize(x, (3, 2), scale=[1, 2, 3], axis=1)}, -1, "field 1 `b`"),
                ({"a": tensor.resize(x, (3, 2), bias=1.0), "b": tensor.cast(x, "float16")}, -4, "field `b`"),
                ({"a": tensor.crops(x, [[0, 0, 1, 1]] * 4, (3, 2), bias=1.0),
                  "b": tensor.resize(x, (3, 2))}, -4, "field `b`")):
            with pytest.raises(DoraGpuError) as e:
                a.send_output("out", data)
            assert e.value.code == code and word in str(e.value), str(e.value)
        a.send_output("out", tensor.resize(x, (2, 5), mode="bilinear", bias=1.0), {"k": "last"})
        ev = bnode.next(timeout=5)  # the first thing to arrive after the refusals
        assert ev["metadata"] == {"k": "last"}
        assert ev["value"].equals(tensor.from_numpy_resize(x, (2, 5), mode="bilinear", bias=1.0))
    finally:
        a.close()
        bnode.close()
        d.join()
