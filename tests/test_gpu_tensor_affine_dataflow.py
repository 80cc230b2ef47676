"""Torch tensors in HBM normalised and quantised per channel on send through a dataflow (src and
dst on GPU 0, one receiver without a GPU), the tables float32 tensors in HBM: a 37 x 53 x 3 uint8
frame sent as `cast(frame.permute(2, 0, 1), "float16", scale=s, bias=b, axis=0)`, a float16
(5, 17, 9) tensor sent as `quantize(feat, "int8", scale=per_channel, axis=1)`, and a dict mixing
both with a plain field, synchronously and with `asynchronous=True` followed by `sync()`.  The
scenarios run in one child process, tests/tensor_affine_child.py, which imports torch before
dora_amd so that producer and node share one HIP runtime; each test asserts one scenario of its
report.  A device receiver's tensor.to_torch is zero-copy inside the one sample and equal bit for
bit to `tensor.from_numpy_cast` / `tensor.from_numpy_quantize`; a host receiver's array equals it
too; a host table over device values raises in the producer."""
import json
import os
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(launcher, tmp_path_factory):
    d = tmp_path_factory.mktemp("tensor_affine_dataflow")
    out, log = d / "report.json", d / "child.log"
    pid = launcher.spawn([sys.executable, os.path.join(ROOT, "tests", "tensor_affine_child.py"),
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


def test_a_uint8_frame_arrives_as_normalised_float16_chw(report):
    """Four frames from one tensor, rewritten before and poisoned after every send."""
    _ok(report, "frame")
    assert report["frame"]["messages"] == 4


def test_a_float16_tensor_arrives_quantised_per_channel(report):
    _ok(report, "quantise")
    assert report["quantise"]["messages"] == 2


def test_a_record_mixes_both_with_a_plain_field(report):
    """One message, one launch; an asynchronous send holds the fields and the tables until sync()."""
    _ok(report, "record")
    assert report["record"]["held"] == 6


def test_receiver_without_a_gpu_gets_the_array_of_the_normalised_tensor(report):
    _ok(report, "host_receiver")


def test_a_host_table_over_device_values_raises_in_the_producer(report):
    _ok(report, "host_table")
    assert report["host_table"]["refused"] == 3
