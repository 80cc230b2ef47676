"""Torch tensors in HBM quantised on send through a dataflow (src and dst on GPU 0, one receiver
without a GPU): a (3, 48, 64) float16 map in [0, 1] permuted to HWC sent as
`quantize(x.permute(1, 2, 0), torch.uint8, scale=255)`, a (48, 64) float32 depth map sent as uint16
millimetres (a NaN, an infinity and everything past 65.535 m included), and the mixed record
`{"mask": quantize(f32, "uint8", 255), "feat": cast(bf16, "float32"), "ids": int64}`, synchronously
and with `asynchronous=True` followed by `sync()`.  The scenarios run in one child process,
tests/tensor_quant_child.py, which imports torch before dora_amd so that producer and node share
one HIP runtime; each test asserts one scenario of its report.  A device receiver's
tensor.to_torch is zero-copy inside the one sample; every field, and a host receiver's pyarrow
array, equals tensor.from_numpy_quantize of the source."""
import json
import os
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(launcher, tmp_path_factory):
    d = tmp_path_factory.mktemp("tensor_quant_dataflow")
    out, log = d / "report.json", d / "child.log"
    pid = launcher.spawn([sys.executable, os.path.join(ROOT, "tests", "tensor_quant_child.py"),
                          str(out)], out=str(log))
    deadline = time.monotonic() + 240
    while launcher.poll(pid) is None:
        if time.monotonic() > deadline:
            launcher.kill(pid)
            pytest.fail("the torch child did not finish:\n" + log.read_text()[-3000:])
        time.sleep(0.05)
    if not out.exists():
        pytest.fail("the torch child wrote no report:\n" + log.read_text()[-3000:])
    return json.loads(out.read_text())


def _ok(report, name):
    assert "setup" not in report, report["setup"].get("error")
    assert name in report, f"scenario {name} did not run: {sorted(report)}"
    assert report[name]["ok"], report[name].get("error")


def test_a_float16_map_arrives_as_uint8_hwc(report):
    """Three maps from one tensor, rewritten before and overwritten after every send."""
    _ok(report, "mask")
    assert report["mask"]["messages"] == 3


def test_a_float32_depth_map_arrives_as_uint16_millimetres(report):
    _ok(report, "depth")
    assert report["depth"]["messages"] == 2


def test_a_record_mixes_quantised_cast_and_plain_fields(report):
    """One message, one launch; an asynchronous send holds all three fields until sync()."""
    _ok(report, "record")
    assert report["record"]["held"] == 3


def test_receiver_without_a_gpu_gets_the_array_of_the_quantised_tensor(report):
    _ok(report, "host_receiver")
