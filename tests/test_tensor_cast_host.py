"""Cast sends on the CPU (no GPU): `Node.send_output(output_id, tensor.cast(x, dtype, scale))`, bare
and as fields of a dict next to plain fields, of numpy and CPU torch values (bfloat16 included)
through a host-only two-node dataflow arrives as the pyarrow array of tensor.from_numpy_cast with
the oracle's type info; and the CPU's conversions, the plain-integer float32 -> float16 and
float16 -> float32 of cast_device.h among them, are checked through the host plan over their
whole domain: around every float16 (exact values, midpoints, midpoints +-1 ulp), every float16 and
bfloat16 bit pattern, every 8- and 16-bit integer under scales that reach the float16
subnormals, and the float sources under scales whose products land in the float16 and float32
subnormals, are zero of either sign, or overflow."""
import ctypes

import numpy as np
import pyarrow as pa
import pytest

from dora_amd import tensor
from dora_amd._lib import ARROW_DEVICE_CPU, DoraGpuError
from oracle.pack_ref import pack
from tests import cast_records as cr
from tests.test_dataflow_host import InProcessDaemon, _start_nodes

DESC = {"nodes": [
    {"id": "src", "outputs": ["out"]},
    {"id": "dst", "inputs": {"in": {"source": "src/out", "queue_size": 100}}, "outputs": []},
]}


def nan_equal(got, want):
    """pyarrow arrays of one type, equal value for value, NaN for NaN."""
    assert got.type == want.type and len(got) == len(want)
    g, w = tensor.to_numpy(got), tensor.to_numpy(want)
    if isinstance(w, dict):
        assert list(g) == list(w)
        return all(np.array_equal(g[k], w[k], equal_nan=w[k].dtype.kind == "f") for k in w)
    return np.array_equal(g, w, equal_nan=True)


def test_host_dataflow_delivers_casts(lib):
    import torch
    frame = cr.source("uint8", (6, 8, 3))
    mic = cr.source("int16", (1600,))
    half = cr.source("float16", (50, 4))
    bf = torch.randn(40, 6).to(torch.bfloat16)
    bf_bits = bf.view(torch.int16).numpy().view(np.uint16)
    conf = cr.source("float32", (6,))
    ro = np.broadcast_to(np.arange(5, dtype=np.uint8), (6, 5))  # read-only: no capsule
    big = cr.source("uint8", (64, 64, 3))
    s255, s32k = 1 / 255, 1 / 32768
    sent = [  # (what is sent, the pyarrow array it must arrive as)
        (tensor.cast(frame.transpose(2, 0, 1), "float16", scale=s255),
         tensor.from_numpy_cast(frame.transpose(2, 0, 1), "float16", s255)),
        (tensor.cast(mic, np.float32, scale=s32k), tensor.from_numpy_cast(mic, "float32", s32k)),
        (tensor.cast(half, "float32"), tensor.from_numpy_cast(half, "float32")),
        (tensor.cast(bf, torch.float32), tensor.from_numpy_cast(bf_bits, "float32", bfloat16=True)),
        (tensor.cast(torch.from_numpy(frame), torch.float16, scale=s255),
         tensor.from_numpy_cast(frame, "float16", s255)),
        (tensor.cast(ro, "float32", scale=2.0), tensor.from_numpy_cast(ro, "float32", 2.0)),
        (tensor.cast(big, "float32", scale=s255), tensor.from_numpy_cast(big, "float32", s255)),
        (tensor.cast(conf, "float32"), tensor.from_numpy(conf)),  # the identity: the plain tensor
        ({"image": tensor.cast(frame, "float16", scale=s255), "conf": conf},
         pa.StructArray.from_arrays([tensor.from_numpy_cast(frame, "float16", s255),
                                     tensor.from_numpy(conf)], names=["image", "conf"])),
        ({"n": conf, "same": tensor.cast(ro, "float16"), "x": tensor.cast(conf, "float16", scale=3)},
         pa.StructArray.from_arrays([tensor.from_numpy(conf), tensor.from_numpy_cast(ro, "float16"),
                                     tensor.from_numpy_cast(conf, "float16", 3)],
                                    names=["n", "same", "x"])),
    ]
    assert len(pack(sent[0][1])[0]) < 4096 <= len(pack(sent[6][1])[0])  # inline and shared memory
    d = InProcessDaemon(DESC)
    nodes = _start_nodes(d.shm, ["src", "dst"])
    a, b = nodes["src"], nodes["dst"]
    try:
        for k, (data, _) in enumerate(sent):
            a.send_output("out", data, {"k": k})
        for k, (_, want) in enumerate(sent):
            ev = b.next(timeout=5)
            assert ev["type"] == "INPUT" and ev["metadata"] == {"k": k}
            got = ev["value"]
            got.validate(full=True)
            assert nan_equal(got, want), k
            assert ev["type_info"].to_json() == pack(want)[1].to_json(), k
        # refusals: nothing leaves
        for data, code, word in (
                (tensor.cast(np.zeros(4, np.int32), "float32"), -4, "int32"),
                (tensor.cast(np.zeros(4, np.float64), "float16"), -4, "float64"),
                (tensor.cast(mic, "int32"), -4, "destination"),
                (tensor.cast(mic, torch.bfloat16), -4, "bfloat16"),
                (tensor.cast(mic, "float32", scale=float("nan")), -1, "scale"),
                ({"a": conf, "b": tensor.cast(np.zeros(6, np.int64), "float32")}, -4, "field 1 `b`"),
                ({"a": conf, "b": tensor.cast(mic, "float32")}, -1, "leading extent")):
            with pytest.raises(DoraGpuError) as e:
                a.send_output("out", data)
            assert e.value.code == code and word in str(e.value), str(e.value)
        with pytest.raises(DoraGpuError) as e:  # a torch bfloat16 tensor is no tensor message
            a.send_output("out", bf)
        assert e.value.code == -4 and "bfloat16" in str(e.value)
        with pytest.raises(TypeError) as e:
            a.send_output("out", object())
        assert "cast" in str(e.value)
        a.send_output("out", tensor.cast(mic[:3], "float32"), {"k": "last"})
        ev = b.next(timeout=5)  # the first thing to arrive after the refusals
        assert ev["metadata"] == {"k": "last"}
        assert ev["value"].equals(tensor.from_numpy_cast(mic[:3], "float32"))
    finally:
        a.close()
        b.close()
        d.join()


@pytest.fixture(scope="module")
def sets():
    return cr.value_sets()


def test_value_sets_cover_what_they_claim(sets):
    by = {label: x for label, x, _ in sets}
    r = by["f32->f16 rounding"]
    assert len(r) == 4 * 63488 + 18 and np.isnan(r).sum() == 4
    for v in (65504.0, 65520.0, np.float32(65519.996)):
        assert (r == np.float32(v)).any()
    assert len(by["f16->f32 all"]) == len(by["bf16->f32 all"]) == 65536
    assert len(sets) == cr.N_VALUE_SETS and len({label for label, _, _ in sets}) == len(sets)
    assert [label for label, _, _ in sets[:3]] == ["f32->f16 rounding", "f16->f32 all", "bf16->f32 all"]
    # scaled float sources: products inside the float16 and the float32 subnormals, rounded
    # there, zero products of both signs, overflow, and a scale that is itself subnormal
    def results(label):
        _, x, c = next(t for t in sets if t[0] == label)
        return cr.to_f32(x, c["src"]), cr.want(x, c)
    x, y = results("float16->float16 * 6.103515625e-05")
    assert ((y != 0) & (np.abs(y) < 2.0 ** -14)).any()
    x, y = results("bfloat16->float32 * 7.52316384526264e-37")
    assert ((y != 0) & (np.abs(y) < 2.0 ** -126)).any() and ((y == 0) & (x != 0)).any()
    for label in ("float16->float32 * 0.0", "bfloat16->float16 * -0.0", "float16->float16 * -1.0"):
        x, y = results(label)
        zero = y == 0
        assert (np.signbit(y[zero])).any() and (~np.signbit(y[zero])).any(), label
    x, y = results(f"f32->f32 f16 values * {cr.F32_SCALES[0]!r}")
    sub = (y != 0) & (np.abs(y) < 2.0 ** -126)
    with np.errstate(invalid="ignore"):  # (the signalling NaNs among the inputs)
        exact = x.astype(np.float64) * np.float64(np.float32(cr.F32_SCALES[0]))
    assert sub.sum() > 1000 and (y[sub].astype(np.float64) != exact[sub]).any()  # rounded there
    x, y = results(f"f32->f32 f16 values * {cr.F32_SCALES[1]!r}")
    assert (np.isinf(y) & np.isfinite(x)).any()
    assert 0 < cr.F32_SCALES[2] < 2.0 ** -126
    # the smallest scale drives float16 results into the subnormal range
    x = cr.want(cr.all_patterns("uint8"), cr.cast("uint8", "float16", 2.0 ** -20))
    assert ((x != 0) & (np.abs(x) < 2.0 ** -14)).any()


@pytest.mark.parametrize("k", range(cr.N_VALUE_SETS))
def test_host_conversions_over_their_domain(lib, sets, k):
    """Through the host plan (the CPU converts inside the call, dense views included): bit-equal
    to numpy where numpy gives no NaN, a NaN where it does."""
    label, x, c = sets[k]
    rec = [(None, x, x, c)]
    with cr.plan_cast(rec, lambda b: b.__array_interface__["data"][0], ARROW_DEVICE_CPU) as p:
        (ptr, off, n), = p.segments()
        assert off == 0 and n == p.size == x.size * np.dtype(c["dst"]).itemsize
        cr.same(ctypes.string_at(ptr, n), cr.want(x, c), label)
