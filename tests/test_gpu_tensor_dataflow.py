"""torch tensors in HBM through a dataflow (src and dst on GPU 0, a relay in a process of its
own on GPU 0, one receiver without a GPU).  The scenarios run in one child process, tests/tensor_torch_child.py, which imports torch
before dora_amd so that producer and node share one HIP runtime (this process loaded the library
first); each test asserts one scenario of its report.  Received samples are downloaded with
to_pyarrow, so nothing here depends on how a device receiver exports tensors."""
import json
import os
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(launcher, tmp_path_factory):
    d = tmp_path_factory.mktemp("tensor_dataflow")
    out, log = d / "report.json", d / "child.log"
    pid = launcher.spawn([sys.executable, os.path.join(ROOT, "tests", "tensor_torch_child.py"),
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


def test_torch_views_arrive_with_the_oracles_bytes_and_type_info(report):
    """.T, .permute(2, 0, 1), a crop, a dense tensor, 1-D tensors."""
    _ok(report, "views")


def test_source_overwritten_right_after_a_synchronous_send(report):
    """200 messages, t.mul_(k) on torch's stream right before each send and t.fill_(-1) right
    after it returns: the stream handshake and the synchronous wait."""
    _ok(report, "sync_overwrite")
    assert report["sync_overwrite"]["messages"] == 200


def test_source_overwritten_after_sync_of_asynchronous_sends(report):
    _ok(report, "async_overwrite")
    assert report["async_overwrite"]["messages"] == 200


def test_receiver_without_a_gpu_gets_the_nested_host_array(report):
    _ok(report, "host_receiver")


def test_relay_process_sends_a_transposed_view_of_a_received_sample(report):
    """The relay runs in a process of its own: its input is an IPC-opened slot."""
    print("relay process:", report.get("relay", {}).get("relay"))
    _ok(report, "relay")
    assert report["relay"]["relay"]["sent"] and report["relay"]["relay"]["ipc_opens"] >= 1


def test_asynchronous_sends_hold_at_most_the_bound(report):
    _ok(report, "async_bound")
    assert report["async_bound"]["held_max"] == 64


def test_gather_send_is_timed_in_regions_and_by_profiling(report):
    _ok(report, "timing")


def test_refused_tensors_send_nothing_and_the_next_send_arrives(report):
    """A tensor on another GPU is a TypeError naming both; a view beyond its allocation is
    DORA_ERR_INVALID; the next valid send is the next message."""
    _ok(report, "refusals")
