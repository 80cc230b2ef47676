"""Argmax sends on the CPU (no GPU): `Node.send_output(output_id, tensor.argmax(x, axis, dtype))`,
bare and as fields of a dict next to plain fields and other argmax fields, of numpy and CPU torch
values (bfloat16 included) through a host-only two-node dataflow (daemon, receiving node over
shared memory) arrive as the pyarrow array of `tensor.from_numpy_argmax` with the oracle's type
info, bit for bit: every case of tests/argmax_records.py, all 7 sources and all 4 index dtypes,
read-only values included.  What a send refuses raises, nothing leaves, and the next good message
is the first to arrive."""
import numpy as np
import pyarrow as pa
import pytest

from dora_amd import tensor
from dora_amd._lib import DoraGpuError
from oracle.pack_ref import pack
from tests import argmax_records as ar
from tests import cast_records as cr
from tests.test_dataflow_host import InProcessDaemon, _start_nodes
from tests.test_tensor_cast_host import DESC


def as_values(src, x):
    """What a producer holds of source view `x`: bfloat16 as a torch tensor, else numpy."""
    if src != "bfloat16":
        return x
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int16).copy()).view(torch.bfloat16)


def message(rec):
    """(what is sent, the array it must arrive as) of a record of tests/argmax_records.py."""
    send, cols = {}, []
    for name, _, v, r in rec:
        if r is None:
            send[name], col = v, tensor.from_numpy(v)
        else:
            send[name] = tensor.argmax(as_values(r["src"], v), r["axis"], r["dtype"])
            col = tensor.from_numpy_argmax(v, r["axis"], r["dtype"], bfloat16=r["src"] == "bfloat16")
        cols.append(col)
    if len(rec) == 1 and rec[0][0] is None:
        return send[None], cols[0]
    return send, pa.StructArray.from_arrays(cols, names=[r[0] for r in rec])


def test_host_dataflow_delivers_class_maps(lib):
    import torch
    sent = [message(rec) for _, rec, _ in ar.cases()]
    logits = cr.source("float32", (19, 6, 8), seed=3)
    ro = np.broadcast_to(np.arange(5, dtype=np.uint8), (6, 5))  # read-only: no capsule
    bf = torch.from_numpy(cr.source("float32", (7, 33), seed=4)).to(torch.bfloat16)
    bf_bits = bf.view(torch.int16).numpy().view(np.uint16)
    sent += [
        (tensor.argmax(torch.from_numpy(logits), 0, torch.uint8),
         tensor.from_numpy_argmax(logits, 0, "uint8")),
        (tensor.argmax(bf, -1, "int32"), tensor.from_numpy_argmax(bf_bits, -1, "int32", bfloat16=True)),
        (tensor.argmax(ro, 1, np.uint16), tensor.from_numpy_argmax(ro, 1, "uint16")),
        (tensor.argmax(ro, 0), tensor.from_numpy_argmax(ro, 0)),
        ({"cls": tensor.argmax(ro, 1, "uint8"), "ro": ro},
         pa.StructArray.from_arrays([tensor.from_numpy_argmax(ro, 1, "uint8"), tensor.from_numpy(ro)],
                                    names=["cls", "ro"])),
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
            assert got.type == want.type and got.equals(want), k
            assert ev["type_info"].to_json() == pack(want)[1].to_json(), k
        # refusals inside the send: nothing leaves
        x = cr.source("float32", (4, 3))
        for data, code, word in (
                (tensor.argmax(x[0], 0), -1, "dimensions"),
                (tensor.argmax(x, 2), -1, "axis"),
                (tensor.argmax(x, -3), -1, "axis"),
                (tensor.argmax(np.zeros((4, 0), np.float32), 1), -1, "extent 0"),
                (tensor.argmax(np.zeros((2, 257), np.uint8), 1, "uint8"), -1, "256"),
                (tensor.argmax(np.zeros((4, 3), np.float64), 1), -4, "float64"),
                (tensor.argmax(x, 1, "int16"), -4, "int16"),
                (tensor.argmax(x, 1, "float32"), -4, "float32"),
                ({"a": x, "b": tensor.argmax(x, 2)}, -1, "field 1 `b`"),
                ({"a": x, "b": tensor.argmax(x, 0)}, -1, "leading extent"),
                ({"a": tensor.argmax(x, 1), "b": tensor.cast(x, "float16")}, -4, "field `b`"),
                ({"a": tensor.quantize(x, "uint8"), "b": tensor.argmax(x, 1)}, -4, "field `a`")):
            with pytest.raises(DoraGpuError) as e:
                a.send_output("out", data)
            assert e.value.code == code and word in str(e.value), str(e.value)
        a.send_output("out", tensor.argmax(x, 1, "uint8"), {"k": "last"})
        ev = bnode.next(timeout=5)  # the first thing to arrive after the refusals
        assert ev["metadata"] == {"k": "last"}
        assert ev["value"].equals(tensor.from_numpy_argmax(x, 1, "uint8"))
    finally:
        a.close()
        bnode.close()
        d.join()
