"""bench.py as a program on the GPU: a plain run reports the headline alone, and `--dump-outputs`
writes the sample its last timed step delivered (checked against the host restatement of the
seeded payload, dora_amd.workloads.splitmix_bytes)."""
import json
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(launcher, tmp_path, *args):
    """bench.py in a process of its own (spawned by the launcher: this one has HIP open); its
    stdout line."""
    log = tmp_path / "bench.log"
    pid = launcher.spawn([sys.executable, os.path.join(ROOT, "bench.py"), *args,
                          "--detail", str(tmp_path / "detail.json")], out=str(log))
    deadline = time.monotonic() + 120
    while (rc := launcher.poll(pid)) is None:
        if time.monotonic() > deadline:
            launcher.kill(pid)
            pytest.fail("bench.py did not finish:\n" + log.read_text()[-2000:])
        time.sleep(0.02)
    text = log.read_text()
    assert rc == 0, text[-2000:]
    return json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1])


# one ragged size below bench.DUMP_MAX_ELEMS (dumped whole) and one just above (seeded selection)
@pytest.mark.gpu
@pytest.mark.parametrize("size", [1_000_003, (8 << 20) + 5])
def test_plain_run_dumps_its_last_sample(launcher, tmp_path, size):
    import bench
    from dora_amd.workloads import payload_seed, splitmix_bytes
    out = tmp_path / "dump"
    line = _run_bench(launcher, tmp_path, "--gpus", "1", "--steps", "3", "--warmup", "2",
                      "--size", str(size), "--dump-outputs", str(out))
    assert line["steps"] == 3 and line["warmup"] == 2 and line["unit"] == "GB/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["ms_per_step"] > 0
    # value and ms_per_step are one measurement (the line rounds ms_per_step to 1e-4 ms)
    assert line["value"] == pytest.approx(size / (line["ms_per_step"] * 1e-3) / 1e9,
                                          rel=0.5e-4 / line["ms_per_step"] + 1e-3)
    assert line["config"]["msg_bytes"] == size
    # 2 warmup messages checksummed on receipt, the 3 timed ones after the region's ack
    assert line["parity"] == {"verified_msgs": 5, "mismatches": 0}
    # nothing but the headline ran
    for k in ("sync_send", "sync_send_4mb", "mid_us_frac", "c3", "cpu_baseline", "cross_gpu"):
        assert k not in line, k
    assert line["latency_summary"] == {}
    assert os.listdir(out) == ["sample.npy"]
    got = np.load(out / "sample.npy")
    want = np.frombuffer(splitmix_bytes(size, payload_seed(size)), np.uint8)
    if size > bench.DUMP_MAX_ELEMS:
        want = want[np.sort(np.random.default_rng(0xD05A).integers(0, size, bench.DUMP_MAX_ELEMS))]
    assert got.dtype == np.float32 and got.nbytes <= 64 << 20
    assert np.array_equal(got, want.astype(np.float32))
