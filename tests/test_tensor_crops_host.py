"""Crops sends on the CPU (no GPU): `Node.send_output(output_id, tensor.crops(frame, boxes, size,
...))`, bare and as fields of a dict next to plain fields and other crops fields, of numpy and CPU
torch values (bfloat16 included) through a host-only two-node dataflow (daemon, receiving node over
shared memory) arrive as the pyarrow array of `tensor.from_numpy_crops` with the oracle's type
info, bit for bit but for the payload of a NaN: every case of tests/crop_records.py, read-only
values and boxes given as a list included.  What a send refuses raises, nothing leaves, and the
next good message is the first to arrive."""
import numpy as np
import pyarrow as pa
import pytest

from dora_amd import tensor
from dora_amd._lib import DoraGpuError
from oracle.pack_ref import pack
from tests import cast_records as cr
from tests import crop_records as kr
from tests.test_dataflow_host import InProcessDaemon, _start_nodes
from tests.test_tensor_cast_host import DESC
from tests.test_tensor_resize_host import as_values, same_arrays


def message(rec):
    """(what is sent, the array it must arrive as) of a record of tests/crop_records.py."""
    send, cols = {}, []
    for name, _, v, c in rec:
        if c is None:
            send[name], col = v, tensor.from_numpy(v)
        else:
            send[name] = tensor.crops(as_values(c["src"], v), c["boxes"], c["size"], axes=c["axes"],
                                      mode=c["mode"], dtype=c["dst"])
            col = tensor.from_numpy_crops(v, c["boxes"], c["size"], axes=c["axes"], mode=c["mode"],
                                          dtype=c["dst"], bfloat16=c["src"] == "bfloat16")
        cols.append(col)
    if len(rec) == 1 and rec[0][0] is None:
        return send[None], cols[0]
    return send, pa.StructArray.from_arrays(cols, names=[r[0] for r in rec])


def test_host_dataflow_delivers_crops(lib):
    import torch
    sent = [message(rec) for _, rec, _ in kr.cases()]
    frame = cr.source("uint8", (12, 16, 3), seed=3)
    rows = [(1, 2, 9, 11), (-4, 8, 6, 40), (0, 0, 0, 0)]
    bx = np.array(rows, np.int32)
    ro = np.broadcast_to(np.arange(5, dtype=np.uint8), (6, 5))  # read-only: no capsule
    ro_bx = np.array([(0, 0, 6, 5), (2, 1, 5, 4)], np.int32)
    ro_bx.flags.writeable = False
    bf = torch.from_numpy(cr.source("float32", (7, 9), seed=4)).to(torch.bfloat16)
    bf_bits = bf.view(torch.int16).numpy().view(np.uint16)
    sent += [
        (tensor.crops(torch.from_numpy(frame), torch.from_numpy(bx), (5, 7), axes=(0, 1)),
         tensor.from_numpy_crops(frame, bx, (5, 7), axes=(0, 1))),
        (tensor.crops(torch.from_numpy(frame).permute(2, 0, 1), rows, (6, 6), dtype=torch.float16),
         tensor.from_numpy_crops(frame.transpose(2, 0, 1), bx, (6, 6), dtype="float16")),
        (tensor.crops(bf, bx[:2], (3, 4), mode="nearest", dtype="float32"),
         tensor.from_numpy_crops(bf_bits, bx[:2], (3, 4), mode="nearest", dtype="float32", bfloat16=True)),
        (tensor.crops(ro, ro_bx, (3, 9)), tensor.from_numpy_crops(ro, ro_bx, (3, 9))),
        (tensor.crops(frame, ro_bx, (3, 9), axes=(0, 1)),
         tensor.from_numpy_crops(frame, ro_bx, (3, 9), axes=(0, 1))),
        (tensor.crops(frame, [], (3, 9), axes=(0, 1)),
         tensor.from_numpy_crops(frame, [], (3, 9), axes=(0, 1))),
        ({"crop": tensor.crops(ro, ro_bx, (6, 2), dtype=np.int16), "box": ro_bx},
         pa.StructArray.from_arrays([tensor.from_numpy_crops(ro, ro_bx, (6, 2), dtype="int16"),
                                     tensor.from_numpy(ro_bx)], names=["crop", "box"])),
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
        x = cr.source("float32", (4, 3))
        two = np.array([(0, 0, 2, 2), (1, 1, 4, 3)], np.int32)
        for data, code, word in (
                (tensor.crops(x[0], two, (2, 2), axes=(0, 0)), -1, "dimensions"),
                (tensor.crops(np.zeros((1,) * 6 + (4, 3), np.uint8), two, (2, 2)), -1, "8 dimensions"),
                (tensor.crops(x, two, (2, 2), axes=(0, 2)), -1, "axis"),
                (tensor.crops(x, two, (2, 2), axes=(1, 1)), -1, "same dimension"),
                (tensor.crops(x, two, (0, 2)), -1, "extent 0"),
                (tensor.crops(x, two, (2, 32769)), -1, "32769"),
                (tensor.crops(np.zeros((4, 3), np.float64), two, (2, 2)), -4, "float64"),
                (tensor.crops(x, two, (2, 2), dtype="int32"), -4, "int32"),
                (tensor.crops(bf, two, (2, 2)), -4, "bfloat16"),
                (tensor.crops(x, two.astype(np.int64), (2, 2)), -1, "not int32"),
                (tensor.crops(x, two.astype(np.float32), (2, 2)), -1, "not int32"),
                (tensor.crops(x, two.reshape(-1), (2, 2)), -1, "[K, 4]"),
                (tensor.crops(x, np.zeros((2, 5), np.int32), (2, 2)), -1, "[K, 4]"),
                (tensor.crops(x, np.zeros((2, 8), np.int32)[:, ::2], (2, 2)), -1, "dense"),
                (tensor.crops(x, np.zeros((4, 4), np.int32)[::2], (2, 2)), -1, "dense"),
                ({"a": x, "b": tensor.crops(x, two, (4, 2), axes=(0, 2))}, -1, "field 1 `b`"),
                ({"a": x, "b": tensor.crops(x, two, (5, 3))}, -1, "leading extent"),
                ({"a": tensor.crops(x, two, (5, 3)), "b": tensor.crops(x, two[:1], (5, 3))}, -1,
                 "leading extent"),
                ({"a": tensor.crops(x, two, (4, 2)), "b": tensor.cast(x, "float16")}, -4, "field `b`"),
                ({"a": tensor.quantize(x, "uint8"), "b": tensor.crops(x, two, (4, 2))}, -4, "field `a`"),
                ({"a": tensor.argmax(x, 1), "b": tensor.crops(x, two, (4, 2))}, -4, "field `a`"),
                ({"a": tensor.resize(x, (2, 2)), "b": tensor.crops(x, two, (4, 2))}, -4, "field `a`")):
            with pytest.raises(DoraGpuError) as e:
                a.send_output("out", data)
            assert e.value.code == code and word in str(e.value), str(e.value)
        with pytest.raises(DoraGpuError) as e:
            a.send_output("out", {"a": tensor.resize(x, (2, 2)), "b": tensor.crops(x, two, (4, 2))})
        assert "message of its own" in str(e.value)  # what to do instead
        a.send_output("out", tensor.crops(x, two, (2, 5)), {"k": "last"})
        ev = bnode.next(timeout=5)  # the first thing to arrive after the refusals
        assert ev["metadata"] == {"k": "last"}
        assert ev["value"].equals(tensor.from_numpy_crops(x, two, (2, 5)))
    finally:
        a.close()
        bnode.close()
        d.join()
