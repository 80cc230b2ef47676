"""Torch frames in HBM resized on send through a dataflow (src and dst on GPU 0, one receiver
without a GPU): a bare HWC uint8 frame to uint8, bilinear; the same through `permute(2, 0, 1)` to
float16, bilinear; a dict `{"thumb": resize(batch, nearest), "stamp": int64}`, synchronously and
with `asynchronous=True` followed by `sync()`; and a frame in host memory through the CPU path.
The scenarios run in one child process, tests/tensor_resize_child.py, which imports torch before
dora_amd so that producer and node share one HIP runtime; each test asserts one scenario of its
report.  A device receiver's tensor.to_torch is zero-copy inside the one sample and equal to
`tensor.from_numpy_resize`; so is a host receiver's array; what the send refuses raises in the
producer."""
import json
import os
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(launcher, tmp_path_factory):
    d = tmp_path_factory.mktemp("tensor_resize_dataflow")
    out, log = d / "report.json", d / "child.log"
    pid = launcher.spawn([sys.executable, os.path.join(ROOT, "tests", "tensor_resize_child.py"),
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


def test_a_uint8_frame_arrives_resized(report):
    """Three frames from one tensor, rewritten before and poisoned after every send."""
    _ok(report, "hwc")
    assert report["hwc"]["messages"] == 3


def test_a_permuted_frame_arrives_as_float16_planes(report):
    _ok(report, "chw")
    assert report["chw"]["messages"] == 2


def test_a_record_of_thumbnails_and_a_plain_field(report):
    """One message, one launch; an asynchronous send holds both tensors until sync()."""
    _ok(report, "record")
    assert report["record"]["held"] == 2


def test_a_host_frame_takes_the_cpu_path(report):
    _ok(report, "host_source")


def test_refusals_raise_in_the_producer(report):
    _ok(report, "refused")
    assert report["refused"]["refused"] == 7
