"""Ragged batches of torch tensors in HBM through a dataflow as one List message (src and dst on
GPU 0, one receiver without a GPU).  The scenarios run in one child process,
tests/tensor_list_child.py, which imports torch before dora_amd so that producer and node share
one HIP runtime (this process loaded the library first); each test asserts one scenario of its
report.  A device receiver reads the message with tensor.to_torch: a Ragged of kDLROCM tensors
whose data pointers lie inside the one sample."""
import json
import os
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(launcher, tmp_path_factory):
    d = tmp_path_factory.mktemp("tensor_list_dataflow")
    out, log = d / "report.json", d / "child.log"
    pid = launcher.spawn([sys.executable, os.path.join(ROOT, "tests", "tensor_list_child.py"),
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


def test_ragged_batches_rewritten_between_synchronous_sends(report):
    """50 messages from one tensor and its partition, both rewritten before and poisoned after
    every send: a record cut by int64 lengths in HBM, a bare tensor cut by int32 offsets in HBM, a
    record cut by a host list; values, offsets, type info and zero-copy at a device receiver."""
    _ok(report, "sync_rewrite")
    assert report["sync_rewrite"]["messages"] == 50


def test_receiver_without_a_gpu_gets_the_list_array(report):
    _ok(report, "host_receiver")
    assert report["host_receiver"]["messages"] == 2


def test_asynchronous_send_holds_fields_and_partition_until_sync(report):
    _ok(report, "async")
    assert report["async"]["held"] == 5


def test_device_words_that_do_not_describe_the_rows_arrive_clamped(report):
    _ok(report, "clamped")


def test_refused_batches_send_nothing_and_the_next_send_arrives(report):
    """A device partition with host values is a TypeError that says `.tolist()`; a host
    partition short of N is DORA_ERR_INVALID; the next valid batch is the next message, and
    N == 0 with B == 3 and B == 0 arrive as empty lists."""
    _ok(report, "refusals")
