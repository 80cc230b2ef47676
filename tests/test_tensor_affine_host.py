"""Affine sends on the CPU (no GPU): `Node.send_output(output_id, tensor.cast(x, dtype, scale=s,
bias=b, axis=a))` and the same of `tensor.quantize`, bare and as fields of a dict next to a plain,
a cast and a quantised field, of numpy and CPU torch values through a host-only two-node dataflow
(daemon, receiving node) arrive as the pyarrow array of `tensor.from_numpy_cast` /
`tensor.from_numpy_quantize` with the oracle's type info, bit for bit: all 7 sources to float16,
float32, uint8, int8, uint16 and int16, tables as lists, numpy arrays and CPU tensors, read-only
values included.  What a host send refuses — a table of the wrong length, a value that is not
finite, a device-less mix-up of arguments — raises and nothing leaves."""
import numpy as np
import pyarrow as pa
import pytest

from dora_amd import tensor
from dora_amd._lib import DoraGpuError
from oracle.pack_ref import pack
from tests import affine_records as ar
from tests import cast_records as cr
from tests import quant_records as qr
from tests.test_dataflow_host import InProcessDaemon, _start_nodes
from tests.test_tensor_cast_host import DESC

FLOATS, INTS = ("float16", "float32"), ("uint8", "int8", "uint16", "int16")


def bits_equal(got, want):
    """pyarrow arrays of one type, equal bit for bit except where a float is a NaN in both."""
    assert got.type == want.type and len(got) == len(want)
    g, w = tensor.to_numpy(got), tensor.to_numpy(want)
    pairs = [(g[k], w[k]) for k in w] if isinstance(w, dict) else [(g, w)]
    if isinstance(w, dict):
        assert list(g) == list(w)
    for a, b in pairs:
        ar.same(np.ascontiguousarray(a).tobytes(), b)
    return True


def as_values(src, x):
    """What a producer holds of source array `x`: bfloat16 as a torch tensor, else numpy."""
    if src != "bfloat16":
        return x
    import torch
    return torch.from_numpy(x.view(np.int16).copy()).view(torch.bfloat16)


def all_pairs():
    """[(what is sent, the array it must arrive as)]: every source to every destination, a 3-D
    view with the tables along axis 1 (3 channels), under a scale and a bias table."""
    out = []
    s, b = ar.table(3, 1), ar.table(3, 2, "bias")
    for src in cr.SOURCES:
        x = cr.source(src, (4, 3, 5), seed=9)
        bf = src == "bfloat16"
        for dst in FLOATS:
            out.append((tensor.cast(as_values(src, x), dst, scale=s, bias=b, axis=1),
                        tensor.from_numpy_cast(x, dst, s, bfloat16=bf, bias=b, axis=1)))
        for dst in INTS:
            zp = qr.zero_points(dst)[-2]
            out.append((tensor.quantize(as_values(src, x), dst, scale=s, zero_point=zp, bias=b, axis=-2),
                        tensor.from_numpy_quantize(x, dst, s, zp, bfloat16=bf, bias=b, axis=-2)))
    assert len(out) == 7 * 6
    return out


def test_host_dataflow_delivers_affine_conversions(lib):
    import torch
    frame = cr.source("uint8", (6, 8, 3))
    big = cr.source("uint8", (64, 64, 3))
    feat = cr.source("float16", (6, 17, 9))
    conf = cr.source("float32", (6,))
    ro = np.broadcast_to(np.arange(5, dtype=np.uint8), (6, 5))  # read-only: no capsule
    s, b = ar.imagenet()
    per = ar.table(17, 3)
    chw = frame.transpose(2, 0, 1)
    sent = all_pairs() + [
        (tensor.cast(chw, "float16", scale=s, bias=b, axis=0),
         tensor.from_numpy_cast(chw, "float16", s, bias=b, axis=0)),
        (tensor.cast(frame, "float32", scale=s.tolist(), bias=torch.from_numpy(b), axis=-1),
         tensor.from_numpy_cast(frame, "float32", s, bias=b, axis=-1)),
        (tensor.cast(big, "float16", scale=s, bias=b, axis=2),
         tensor.from_numpy_cast(big, "float16", s, bias=b, axis=2)),
        (tensor.quantize(feat, "int8", scale=per, axis=1),
         tensor.from_numpy_quantize(feat, "int8", per, axis=1)),
        (tensor.cast(frame, "float16", scale=1 / 255, bias=-0.5),   # numbers alone, no axis
         tensor.from_numpy_cast(frame, "float16", 1 / 255, bias=-0.5)),
        (tensor.cast(conf, "float32", bias=1.5),                    # to its own dtype: a conversion
         tensor.from_numpy_cast(conf, "float32", bias=1.5)),
        (tensor.cast(frame, "float16", scale=1 / 255, bias=b, axis=2),  # a scalar with a table
         tensor.from_numpy_cast(frame, "float16", 1 / 255, bias=b, axis=2)),
        (tensor.quantize(ro, "uint8", scale=np.arange(5, dtype=np.float32), bias=0.5, axis=1),
         tensor.from_numpy_quantize(ro, "uint8", np.arange(5, dtype=np.float32), bias=0.5, axis=1)),
        ({"image": tensor.cast(chw[None], "float16", scale=s, bias=b, axis=1), "conf": conf[:1],
          "half": tensor.cast(conf[:1], "float16", scale=3),
          "q": tensor.quantize(conf[:1], "uint8", 255)},
         pa.StructArray.from_arrays(
             [tensor.from_numpy_cast(chw[None], "float16", s, bias=b, axis=1),
              tensor.from_numpy(conf[:1]), tensor.from_numpy_cast(conf[:1], "float16", 3),
              tensor.from_numpy_quantize(conf[:1], "uint8", 255)],
             names=["image", "conf", "half", "q"])),
        ({"act": tensor.quantize(feat, "int8", scale=per, axis=1), "ro": ro,
          "n": tensor.cast(ro, "float32", bias=np.ones(5, np.float32), axis=1)},
         pa.StructArray.from_arrays(
             [tensor.from_numpy_quantize(feat, "int8", per, axis=1), tensor.from_numpy(ro),
              tensor.from_numpy_cast(ro, "float32", bias=np.ones(5, np.float32), axis=1)],
             names=["act", "ro", "n"])),
    ]
    d = InProcessDaemon(DESC)
    nodes = _start_nodes(d.shm, ["src", "dst"])
    a, bnode = nodes["src"], nodes["dst"]
    try:
        for k, (data, _) in enumerate(sent):
            a.send_output("out", data, {"k": k})
            ev = bnode.next(timeout=5)
            assert ev["type"] == "INPUT" and ev["metadata"] == {"k": k}
            got, want = ev["value"], sent[k][1]
            got.validate(full=True)
            assert bits_equal(got, want), k
            assert ev["type_info"].to_json() == pack(want)[1].to_json(), k
        # refusals inside the send: nothing leaves
        for data, code, word in (
                (tensor.cast(frame, "float16", scale=[1.0, 2.0], axis=2), -1, "2 elements"),
                (tensor.cast(frame, "float16", bias=[1.0, np.inf, 0.0], axis=2), -1, "not finite"),
                (tensor.cast(frame, "float16", scale=[1.0, np.nan, 0.0], axis=2), -1, "not finite"),
                (tensor.cast(frame, "float16", scale=s, axis=3), -1, "axis"),
                (tensor.cast(frame, "float16", scale=s, axis=-4), -1, "axis"),
                (tensor.cast(frame, "float16", scale=np.ones((3, 1), np.float32), axis=2), -1,
                 "dimensions"),
                (tensor.cast(frame, "float16", bias=float("inf")), -1, "bias"),
                ({"a": conf, "b": tensor.cast(frame, "float16", scale=[1.0], axis=2)}, -1,
                 "field 1 `b`")):
            with pytest.raises(DoraGpuError) as e:
                a.send_output("out", data)
            assert e.value.code == code and word in str(e.value), str(e.value)
        a.send_output("out", tensor.cast(conf[:3], "float32", bias=1.0), {"k": "last"})
        ev = bnode.next(timeout=5)  # the first thing to arrive after the refusals
        assert ev["metadata"] == {"k": "last"}
        assert ev["value"].equals(tensor.from_numpy_cast(conf[:3], "float32", bias=1.0))
    finally:
        a.close()
        bnode.close()
        d.join()


def test_python_refusals_and_unchanged_calls(lib):
    """A table without axis, axis without a table, a vector zero point: TypeError.  Calls without
    bias and axis are what they were: the same entries, the same refusals."""
    x = np.zeros((4, 3), np.float32)
    with pytest.raises(TypeError) as e:
        tensor.quantize(x, "uint8", scale=np.ones(3))
    assert "per-channel" in str(e.value) and "axis=" in str(e.value)
    with pytest.raises(TypeError) as e:
        tensor.cast(x, "float16", bias=np.ones(3))
    assert "axis=" in str(e.value)
    with pytest.raises(TypeError) as e:
        tensor.quantize(x, "uint8", bias=[1.0, 2.0, 3.0])
    assert "axis=" in str(e.value)
    with pytest.raises(TypeError):
        tensor.cast(x, "float16", scale=np.ones(3))  # (as before: float() of an array)
    for make in (lambda: tensor.cast(x, "float16", scale=2.0, axis=1),
                 lambda: tensor.quantize(x, "uint8", scale=2.0, bias=1.0, axis=0),
                 lambda: tensor.cast(x, "float16", axis=1)):
        with pytest.raises(TypeError) as e:
            make()
        assert "axis=" in str(e.value)
    with pytest.raises(TypeError) as e:
        tensor.quantize(x, "uint8", scale=np.ones(3), zero_point=[1, 2, 3], axis=1)
    assert "per-channel" in str(e.value)
    for bad in (tensor.cast(x, "float16", bias=1.0), {"a": x}, tensor.take(x, [0])):
        with pytest.raises(TypeError):
            tensor.quantize(bad, "uint8", bias=1.0)
        with pytest.raises(TypeError):
            tensor.cast(bad, "float16", bias=1.0)
    for wrap in (tensor.ragged, ):
        with pytest.raises(TypeError):
            wrap(tensor.cast(x, "float16", bias=np.ones(3), axis=1), lengths=[4])
    with pytest.raises(TypeError):
        tensor.take(tensor.quantize(x, "int8", scale=np.ones(3), axis=1), [0])
    with pytest.raises(TypeError):
        tensor.masked(tensor.cast(x, "float16", bias=1.0), [1, 0, 1, 1])
    c, q = tensor.cast(x, "float16", scale=0.5), tensor.quantize(x, "uint8", 255, 3)
    assert c._entry() == (2, 16, 0.5) and c._affine() is None
    assert q._entry() == (1, 8, 255.0, 3) and q._affine() is None
    t = tensor.cast(x, "float16", scale=np.ones(3), bias=2, axis=-1)
    assert t.axis == 1 and t.scale is None and t.bias == 2.0 and t._entry() == (2, 16, None)
    with pytest.raises(TypeError):
        tensor.from_numpy_cast(x, "float16", np.ones(3))  # a table needs axis
    with pytest.raises(ValueError):
        tensor.from_numpy_quantize(x, "int8", np.ones(4), axis=1)
