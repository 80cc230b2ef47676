"""Dicts of torch tensors in HBM through a dataflow as one Struct message (src and dst on GPU 0,
one receiver without a GPU).  The scenarios run in one child process,
tests/tensor_struct_child.py, which imports torch before dora_amd so that producer and node share
one HIP runtime (this process loaded the library first); each test asserts one scenario of its
report.  A device receiver reads the message with tensor.to_torch: a dict of kDLROCM tensors over
the one sample."""
import json
import os
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(launcher, tmp_path_factory):
    d = tmp_path_factory.mktemp("tensor_struct_dataflow")
    out, log = d / "report.json", d / "child.log"
    pid = launcher.spawn([sys.executable, os.path.join(ROOT, "tests", "tensor_struct_child.py"),
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


def test_detector_record_rewritten_between_synchronous_sends(report):
    """20 messages of {bbox, conf, cls, ids} from the views of one (67, 6) tensor rewritten before
    and poisoned after every send: shapes, dtypes, values and type info at a device receiver."""
    _ok(report, "sync_rewrite")
    assert report["sync_rewrite"]["messages"] == 20


def test_device_array_fields_export_dlpack(report):
    _ok(report, "fields")


def test_receiver_without_a_gpu_gets_the_struct_array(report):
    _ok(report, "host_receiver")


def test_asynchronous_send_holds_every_field_until_sync(report):
    _ok(report, "async")
    assert report["async"]["held"] == 4


def test_refused_records_send_nothing_and_the_next_send_arrives(report):
    """A dict mixing a numpy array and a device tensor is a TypeError naming both fields; fields
    of different leading extents are DORA_ERR_INVALID; the next valid record is the next message."""
    _ok(report, "refusals")
