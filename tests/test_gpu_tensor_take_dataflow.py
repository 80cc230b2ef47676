"""Rows of torch tensors in HBM taken by an index in HBM through a dataflow (src and dst on GPU 0,
one receiver without a GPU): `take(out[:, :4], keep)`, `take({"bbox": .., "conf": .., "cls": ..},
keep)` and `ragged(take(..), lengths=<int64 tensor in HBM>)` of a (100, 6) float32 `out` and an
int64 `keep` of 0, 1 and 37 words, sent synchronously and with `asynchronous=True` followed by
`sync()`.  The scenarios run in one child process, tests/tensor_take_child.py, which imports torch
before dora_amd so that producer and node share one HIP runtime (this process loaded the library
first); each test asserts one scenario of its report.  A device receiver's tensor.to_torch equals
`out[keep]`, zero-copy inside the one sample, which is byte-equal to the oracle's packing of
tensor.from_numpy_take(..) in every region; a host receiver's array equals that array."""
import json
import os
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(launcher, tmp_path_factory):
    d = tmp_path_factory.mktemp("tensor_take_dataflow")
    out, log = d / "report.json", d / "child.log"
    pid = launcher.spawn([sys.executable, os.path.join(ROOT, "tests", "tensor_take_child.py"),
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


def test_values_and_index_rewritten_between_synchronous_sends(report):
    """50 messages from one tensor, one index and one tensor of counts, all rewritten before and
    poisoned after every send: no stale or torn row, every kind of message at every K."""
    _ok(report, "sync_rewrite")
    assert report["sync_rewrite"]["messages"] == 50


def test_asynchronous_sends_hold_fields_index_and_partition_until_sync(report):
    _ok(report, "async")
    assert report["async"]["held"] == {"bare": 2, "dict": 4, "ragged": 5}


def test_receiver_without_a_gpu_gets_the_array_of_the_indexed_copy(report):
    _ok(report, "host_receiver")
    assert report["host_receiver"]["messages"] == 9


def test_words_that_are_no_row_arrive_as_rows_of_zeros(report):
    _ok(report, "zero_rows")


def test_refused_takes_send_nothing_and_the_next_send_arrives(report):
    """An index away from its values is a TypeError that says to move it; a host partition of the
    N source rows and a float index are DORA_ERR_INVALID; the next valid take is the next
    message."""
    _ok(report, "refusals")
