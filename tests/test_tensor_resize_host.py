"""Resize sends on the CPU (no GPU): `Node.send_output(output_id, tensor.resize(x, size, ...))`,
bare and as fields of a dict next to plain fields and other resize fields, of numpy and CPU torch
values (bfloat16 included) through a host-only two-node dataflow (daemon, receiving node over
shared memory) arrive as the pyarrow array of `tensor.from_numpy_resize` with the oracle's type
info, bit for bit but for the payload of a NaN: every case of tests/resize_records.py, all 7
sources and all 6 destinations, read-only values included.  What a send refuses raises, nothing
leaves, and the next good message is the first to arrive."""
import numpy as np
import pyarrow as pa
import pytest

from dora_amd import tensor
from dora_amd._lib import DoraGpuError
from oracle.pack_ref import pack
from tests import cast_records as cr
from tests import resize_records as rr
from tests.test_dataflow_host import InProcessDaemon, _start_nodes
from tests.test_tensor_cast_host import DESC


def as_values(src, x):
    """What a producer holds of source view `x`: bfloat16 as a torch tensor, else numpy."""
    if src != "bfloat16":
        return x
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int16).copy()).view(torch.bfloat16)


def message(rec):
    """(what is sent, the array it must arrive as) of a record of tests/resize_records.py."""
    send, cols = {}, []
    for name, _, v, r in rec:
        if r is None:
            send[name], col = v, tensor.from_numpy(v)
        else:
            send[name] = tensor.resize(as_values(r["src"], v), r["size"], axes=r["axes"],
                                       mode=r["mode"], dtype=r["dst"])
            col = tensor.from_numpy_resize(v, r["size"], axes=r["axes"], mode=r["mode"],
                                           dtype=r["dst"], bfloat16=r["src"] == "bfloat16")
        cols.append(col)
    if len(rec) == 1 and rec[0][0] is None:
        return send[None], cols[0]
    return send, pa.StructArray.from_arrays(cols, names=[r[0] for r in rec])


def leaf_bytes(arr):
    """The leaf values of a nested tensor array (or of each field of a struct of them) as numpy."""
    if pa.types.is_struct(arr.type):
        return [leaf_bytes(arr.field(i)) for i in range(arr.type.num_fields)]
    while pa.types.is_fixed_size_list(arr.type):
        arr = arr.flatten()
    return [arr.to_numpy(zero_copy_only=False)]


def same_arrays(got, want, what):
    """Equal type and values bit for bit, NaN for NaN (whatever its payload)."""
    assert got.type == want.type and len(got) == len(want), what
    flat = lambda xs: [a for x in xs for a in (flat(x) if isinstance(x, list) else [x])]
    for g, w in zip(flat(leaf_bytes(got)), flat(leaf_bytes(want))):
        rr.same(np.ascontiguousarray(g).tobytes(), w, what)


def test_host_dataflow_delivers_resized_frames(lib):
    import torch
    sent = [message(rec) for _, rec, _ in rr.cases()]
    frame = cr.source("uint8", (12, 16, 3), seed=3)
    ro = np.broadcast_to(np.arange(5, dtype=np.uint8), (6, 5))  # read-only: no capsule
    bf = torch.from_numpy(cr.source("float32", (7, 9), seed=4)).to(torch.bfloat16)
    bf_bits = bf.view(torch.int16).numpy().view(np.uint16)
    sent += [
        (tensor.resize(torch.from_numpy(frame), (5, 7), axes=(0, 1), mode="bilinear"),
         tensor.from_numpy_resize(frame, (5, 7), axes=(0, 1), mode="bilinear")),
        (tensor.resize(torch.from_numpy(frame).permute(2, 0, 1), (6, 6), mode="bilinear",
                       dtype=torch.float16),
         tensor.from_numpy_resize(frame.transpose(2, 0, 1), (6, 6), mode="bilinear", dtype="float16")),
        (tensor.resize(bf, (3, 4), dtype="float32"),
         tensor.from_numpy_resize(bf_bits, (3, 4), dtype="float32", bfloat16=True)),
        (tensor.resize(ro, (3, 9), mode="bilinear"), tensor.from_numpy_resize(ro, (3, 9), mode="bilinear")),
        ({"thumb": tensor.resize(ro, (6, 2), dtype=np.int16), "ro": ro},
         pa.StructArray.from_arrays([tensor.from_numpy_resize(ro, (6, 2), dtype="int16"),
                                     tensor.from_numpy(ro)], names=["thumb", "ro"])),
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
        for data, code, word in (
                (tensor.resize(x[0], (2, 2), axes=(0, 0)), -1, "dimensions"),
                (tensor.resize(x, (2, 2), axes=(0, 2)), -1, "axis"),
                (tensor.resize(x, (2, 2), axes=(-3, 1)), -1, "axis"),
                (tensor.resize(x, (2, 2), axes=(1, 1)), -1, "same dimension"),
                (tensor.resize(x, (0, 2)), -1, "extent 0"),
                (tensor.resize(x, (2, 32769)), -1, "32769"),
                (tensor.resize(np.zeros((4, 3), np.float64), (2, 2)), -4, "float64"),
                (tensor.resize(x, (2, 2), dtype="int32"), -4, "int32"),
                (tensor.resize(x, (2, 2), dtype=torch.bfloat16), -4, "bfloat16"),
                (tensor.resize(bf, (2, 2)), -4, "bfloat16"),
                ({"a": x, "b": tensor.resize(x, (4, 2), axes=(0, 2))}, -1, "field 1 `b`"),
                ({"a": x, "b": tensor.resize(x, (5, 3))}, -1, "leading extent"),
                ({"a": tensor.resize(x, (4, 2)), "b": tensor.cast(x, "float16")}, -4, "field `b`"),
                ({"a": tensor.quantize(x, "uint8"), "b": tensor.resize(x, (4, 2))}, -4, "field `a`"),
                ({"a": tensor.argmax(x, 1), "b": tensor.resize(x, (4, 2))}, -4, "field `a`")):
            with pytest.raises(DoraGpuError) as e:
                a.send_output("out", data)
            assert e.value.code == code and word in str(e.value), str(e.value)
        a.send_output("out", tensor.resize(x, (2, 5), mode="bilinear"), {"k": "last"})
        ev = bnode.next(timeout=5)  # the first thing to arrive after the refusals
        assert ev["metadata"] == {"k": "last"}
        assert ev["value"].equals(tensor.from_numpy_resize(x, (2, 5), mode="bilinear"))
    finally:
        a.close()
        bnode.close()
        d.join()
