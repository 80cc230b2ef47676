"""Boxes in HBM cut from a torch frame in HBM and resized on send through a dataflow (src and dst on
GPU 0, one receiver without a GPU): bare crops of an HWC uint8 frame to uint8 and, through
`permute(2, 0, 1)`, to float16; a dict `{"crop": crops, "box": the boxes, "cls": int64}`,
synchronously and with `asynchronous=True` followed by `sync()`; a host receiver; and frame and
boxes in host memory through the CPU path.  While it sends, the producer's `.cpu()`, `.item()`,
`.tolist()` and `.numpy()` raise for the boxes: they are never read on the host.  The scenarios run
in one child process, tests/tensor_crops_child.py, which imports torch before dora_amd so that
producer and node share one HIP runtime; each test asserts one scenario of its report.  A device
receiver's tensor.to_torch is zero-copy inside the one sample and equal to
`tensor.from_numpy_crops`; what the send refuses raises in the producer."""
import json
import os
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(launcher, tmp_path_factory):
    d = tmp_path_factory.mktemp("tensor_crops_dataflow")
    out, log = d / "report.json", d / "child.log"
    pid = launcher.spawn([sys.executable, os.path.join(ROOT, "tests", "tensor_crops_child.py"),
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


def test_bare_crops_arrive_as_one_tensor(report):
    """Three messages from one frame and one boxes tensor, both rewritten before and poisoned
    after every send, the third through a permuted view to float16."""
    _ok(report, "bare")
    assert report["bare"]["messages"] == 3


def test_a_record_of_crops_boxes_and_classes(report):
    """One message, one launch; an asynchronous send holds the three fields and the crops' boxes
    until sync()."""
    _ok(report, "record")
    assert report["record"]["held"] == 4


def test_a_host_receiver_and_a_host_source(report):
    _ok(report, "host_receiver")


def test_refusals_raise_in_the_producer(report):
    _ok(report, "refused")
    assert report["refused"]["refused"] == 10 and report["refused"]["sides"] == 3
