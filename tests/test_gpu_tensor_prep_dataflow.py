"""Model inputs through a dataflow (src and dst on GPU 0, one receiver without a GPU): a torch
frame in HBM sent through `permute(2, 0, 1)` letterboxed and normalised by per-channel tables in
HBM as one CHW float16 tensor; a dict `{"crop": tensor.crops(.., scale=s, bias=b, axis=2), "box":
boxes}`, synchronously and with `asynchronous=True` followed by `sync()`; a host receiver; and
frame and tables in host memory through the CPU path.  The sender rewrites frame, boxes and tables
after `send_output` returns without changing what arrives, and while it sends, the producer's
`.cpu()`, `.item()`, `.tolist()` and `.numpy()` raise for the tables: they are never read on the
host.  The scenarios run in one child process, tests/tensor_prep_child.py, which imports torch
before dora_amd so that producer and node share one HIP runtime; each test asserts one scenario of
its report.  A device receiver's tensor.to_torch is zero-copy inside the one sample and equal to
the statement; what the send refuses raises in the producer."""
import json
import os
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(launcher, tmp_path_factory):
    d = tmp_path_factory.mktemp("tensor_prep_dataflow")
    out, log = d / "report.json", d / "child.log"
    pid = launcher.spawn([sys.executable, os.path.join(ROOT, "tests", "tensor_prep_child.py"),
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


def test_a_letterboxed_normalised_frame_arrives_as_one_tensor(report):
    """Three messages from one frame and one pair of tables, all rewritten before and poisoned
    after every send."""
    _ok(report, "letterbox")
    assert report["letterbox"]["messages"] == 3


def test_a_record_of_normalised_crops_and_boxes(report):
    """One message, one launch; an asynchronous send holds the two fields, the crops' boxes and
    the two tables until sync()."""
    _ok(report, "record")
    assert report["record"]["held"] == 5


def test_a_host_receiver_and_a_host_source(report):
    _ok(report, "host_receiver")


def test_refusals_raise_in_the_producer(report):
    _ok(report, "refused")
    assert report["refused"]["refused"] == 5 and report["refused"]["sides"] == 2
