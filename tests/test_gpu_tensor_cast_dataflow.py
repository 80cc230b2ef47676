"""Torch tensors in HBM converted on send through a dataflow (src and dst on GPU 0, one receiver
without a GPU): a uint8 6 x 8 x 3 frame sent as `cast(frame.permute(2, 0, 1), torch.float16,
scale=1/255)`, a bfloat16 tensor sent as float32 (dense and as strided views), and the mixed record
`{"image": cast(img, "float16", scale=1/255), "conf": conf}`, synchronously and with
`asynchronous=True` followed by `sync()`.  The scenarios run in one child process,
tests/tensor_cast_child.py, which imports torch before dora_amd so that producer and node share
one HIP runtime (this process loaded the library first); each test asserts one scenario of its
report.  A device receiver's tensor.to_torch is zero-copy inside the one sample and equal to
torch's own `x.float().mul(s).to(dst)` computed on the CPU; a host receiver's array equals
tensor.from_numpy_cast."""
import json
import os
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(launcher, tmp_path_factory):
    d = tmp_path_factory.mktemp("tensor_cast_dataflow")
    out, log = d / "report.json", d / "child.log"
    pid = launcher.spawn([sys.executable, os.path.join(ROOT, "tests", "tensor_cast_child.py"),
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


def test_a_uint8_frame_arrives_as_float16_chw(report):
    """Six frames from one tensor, rewritten before and poisoned after every send."""
    _ok(report, "frame")
    assert report["frame"]["messages"] == 6


def test_a_bfloat16_tensor_arrives_as_float32(report):
    _ok(report, "bfloat16")
    assert report["bfloat16"]["messages"] == 3


def test_a_record_mixes_converted_and_plain_fields(report):
    """One message, one launch; an asynchronous send holds both fields until sync()."""
    _ok(report, "record")
    assert report["record"]["held"] == 2


def test_receiver_without_a_gpu_gets_the_array_of_the_converted_tensor(report):
    _ok(report, "host_receiver")
