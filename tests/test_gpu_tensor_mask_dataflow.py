"""Rows of torch tensors in HBM selected by a bool mask in HBM through a dataflow (src and dst on
GPU 0, one receiver without a GPU): `masked(out[:, :4], keep)`, `masked({"bbox": .., "conf": ..,
"cls": ..}, keep)` and `ragged(masked(..), lengths=<int64 tensor in HBM>)` of a (300, 6) float32
`out`, sent synchronously and with `asynchronous=True` in bursts of 8 followed by `sync()`.  The
scenarios run in one child process, tests/tensor_mask_child.py, which imports torch before
dora_amd so that producer and node share one HIP runtime (this process loaded the library first);
each test asserts one scenario of its report.  A device receiver's sample is byte-equal to the
oracle's packing of tensor.from_numpy_masked(..) in every region and exactly as long — the
workspace behind it does not travel — and its tensor.to_torch gives the N-row values zero-copy,
the first offsets[-1] rows the selected ones; a host receiver's array equals that array."""
import json
import os
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(launcher, tmp_path_factory):
    d = tmp_path_factory.mktemp("tensor_mask_dataflow")
    out, log = d / "report.json", d / "child.log"
    pid = launcher.spawn([sys.executable, os.path.join(ROOT, "tests", "tensor_mask_child.py"),
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


def test_values_and_mask_rewritten_between_synchronous_sends(report):
    """42 messages from one tensor, one mask and one tensor of counts, all rewritten before and
    poisoned after every send: no stale or torn row, every kind of message under every mask."""
    _ok(report, "sync_rewrite")
    assert report["sync_rewrite"]["messages"] == 42


def test_asynchronous_bursts_hold_fields_mask_and_partition_until_sync(report):
    _ok(report, "async_bursts")
    assert report["async_bursts"]["held"] == {"tensor": 2, "record": 4, "ragged": 5}
    assert report["async_bursts"]["messages"] == 24


def test_receiver_without_a_gpu_gets_the_array_of_from_numpy_masked(report):
    _ok(report, "host_receiver")
    assert report["host_receiver"]["messages"] == 9


def test_a_partition_that_does_not_describe_the_rows_is_clamped_through_the_counts(report):
    _ok(report, "garbage_partition")


def test_refused_masks_send_nothing_and_the_next_send_arrives(report):
    """A mask away from its values is a TypeError that says to move it; a host partition of the
    K selected rows, an int32 mask, a mask of another length and a strided one are
    DORA_ERR_INVALID; the next valid mask is the next message."""
    _ok(report, "refusals")
