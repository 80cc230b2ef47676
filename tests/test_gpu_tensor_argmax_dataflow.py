"""Torch logits in HBM reduced to class maps on send through a dataflow (src and dst on GPU 0, one
receiver without a GPU): float16 (19, 64, 96) along 0 to uint8, bfloat16 (33, 1000) along -1 to
int32, and a dict `{"cls": argmax(..), "depth": strided float32}`, synchronously and with
`asynchronous=True` followed by `sync()`.  The scenarios run in one child process,
tests/tensor_argmax_child.py, which imports torch before dora_amd so that producer and node share
one HIP runtime; each test asserts one scenario of its report.  A device receiver's
tensor.to_torch is zero-copy inside the one sample and equal to `torch.argmax(..).to(dtype)`; a
host receiver's array equals `tensor.from_numpy_argmax`; what the send refuses raises in the
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
    d = tmp_path_factory.mktemp("tensor_argmax_dataflow")
    out, log = d / "report.json", d / "child.log"
    pid = launcher.spawn([sys.executable, os.path.join(ROOT, "tests", "tensor_argmax_child.py"),
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


def test_float16_logits_arrive_as_a_uint8_class_map(report):
    """Three maps from one tensor, rewritten before and poisoned after every send."""
    _ok(report, "segmentation")
    assert report["segmentation"]["messages"] == 3


def test_bfloat16_classifier_logits_arrive_as_int32_top1(report):
    _ok(report, "classifier")
    assert report["classifier"]["messages"] == 2


def test_a_record_of_a_class_map_and_a_strided_field(report):
    """One message, one launch; an asynchronous send holds both tensors until sync()."""
    _ok(report, "record")
    assert report["record"]["held"] == 2


def test_receiver_without_a_gpu_gets_the_array_of_the_index_tensor(report):
    _ok(report, "host_receiver")


def test_refusals_raise_in_the_producer(report):
    _ok(report, "refused")
    assert report["refused"]["refused"] == 5
