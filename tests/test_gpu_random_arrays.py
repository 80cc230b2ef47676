"""Seeded random Arrow arrays (tests/random_arrays.py) through both plans on the GPU: the copy
segments through pack_kernel and the transform segments of compacting plans through
transform_kernel, byte for byte against the references the CPU sweep
(tests/test_random_arrays_host.py) holds the emulation to.

* `DeviceArray.from_pyarrow` -> `Plan.of` -> `pack` into a poisoned buffer with 48 bytes of slack,
  the first 200 seeds, once per layout: size, type info, every region, and the poison everywhere
  else.
* The limit cases that are real arrays: every op at 4095, 4096, 4097 and 2 * 4096 + 1 elements
  (blocks past a segment's first), every (bit offset, len mod 8), 40 transform segments (the
  second launch), three blocks before segments of one; and packs to `dst + 1`, `+ 2` and `+ 4`,
  which dora_gpu_pack accepts: rebase's byte-wise branch.
* Node level: 10 seeds with `set_compact(False)` and 10 with `set_compact(True)` from a sending
  node to a receiving node as device arrays — the received array equals the sent slice, and in
  compact mode has offset 0 at every level.
"""
import threading

import pyarrow as pa
import pytest

from tests import random_arrays as ra

pytestmark = pytest.mark.gpu

GPU_SEEDS = 200


@pytest.fixture(scope="module")
def dev():
    from dora_amd import device
    assert device.device_count() >= 1
    device.set_device(0)
    s = device.Stream()
    yield s
    s.close()


def check_on_device(arr, compact, stream, label, shift=0):
    """Pack `arr` at `shift` bytes into a poisoned device buffer and hold it against the layout's
    reference; the bytes before the sample and past its slack keep the poison as well."""
    from dora_amd.arrow_utils import Plan
    from dora_amd.device import DeviceArray, DeviceBuffer
    want, info = ra.reference(arr, compact)
    da = DeviceArray.from_pyarrow(arr)
    plan = Plan.of(da, compact=compact)
    n = plan.size
    buf = DeviceBuffer(shift + n + ra.SLACK + 8)
    try:
        buf.fill(ra.POISON, stream)
        plan.pack(buf.ptr + shift, n + ra.SLACK, stream)
        stream.sync()
        ti = plan.type_info()
        got = buf.to_bytes()
    finally:
        plan.close(); buf.free(); da.close()
    assert n == len(want), (label, n, len(want))
    if compact:
        assert ra.mask_validity(ti) == ra.mask_validity(info), label
    else:
        assert ti.to_json() == info.to_json(), label
    assert got[:shift] == bytes([ra.POISON]) * shift, (label, "bytes before the sample written")
    ra.compare(got[shift:], want, info, compact, label=label)


@pytest.mark.parametrize("compact", [False, True], ids=["reference", "compact"])
def test_every_seed_on_the_device(dev, compact):
    for seed in range(GPU_SEEDS):
        check_on_device(ra.array(seed), compact, dev, seed)


LIMITS = ra.limit_arrays()


def test_limit_arrays_on_the_device(dev):
    for label, arr in LIMITS:
        check_on_device(arr, True, dev, label)
        check_on_device(arr, False, dev, label)


@pytest.mark.parametrize("shift", [1, 2, 4])
def test_compact_pack_to_an_odd_destination(dev, shift):
    """Offsets rebased into a sample at 1, 2 and 4 mod 8 (int64 offsets at 4: still byte-wise),
    bitmaps shifted into it, over more than one block and more than one launch."""
    picked = [(l, a) for l, a in LIMITS
              if l.startswith(("rebase32 4097", "rebase64 4097", "bitshift 4097", "40 ", "three"))]
    assert len(picked) == 5
    for label, arr in picked:
        check_on_device(arr, True, dev, (label, shift), shift=shift)


def node_seeds():
    """Two lists of 10 seeds with a non-empty sample, each holding nulls that are kept, a list and
    a dictionary."""
    out = []
    for first in (0, 100):
        need = {"nulls": 3, "list": 3, "dict": 3}
        got = []
        for seed in range(first, first + 100):
            arr = ra.array(seed)
            if len(arr) == 0 or len(arr) > ra.SMALL or not ra.reference(arr, False)[0]:
                continue
            ns = ra.nodes(arr)
            has = {"nulls": ns[0]["bitmap"] and ns[0]["nulls"] > 0,
                   "list": any(x["fmt"] in ("+l", "+L") for x in ns),
                   "dict": any(x["dict_values"] for x in ns)}
            want = [k for k, v in has.items() if v and need[k] > 0]
            if want or (len(got) + sum(need.values()) < 10):
                for k in want:
                    need[k] -= 1
                got.append(seed)
            if len(got) == 10:
                break
        assert len(got) == 10 and not any(v > 0 for v in need.values()), (got, need)
        out.append(got)
    return out


@pytest.mark.parametrize("compact", [False, True], ids=["reference", "compact"])
def test_seeds_from_node_to_node(launcher, compact):
    """`set_compact` at the node: the reference layout with the validity bitmaps in the sample's
    tail (planned by the collecting and replaying walk where the plan reads device bytes), or the
    compacting plan.  The received array equals the sent slice and its type info is the
    layout's; in compact mode every node has offset 0."""
    from dora_amd.dataflow import Dataflow
    from dora_amd.device import DeviceArray
    from dora_amd.node import Node
    seeds = node_seeds()[int(compact)]
    desc = {"nodes": [
        {"id": "src", "path": "dynamic", "outputs": ["x"]},
        {"id": "dst", "path": "dynamic", "inputs": {"x": {"source": "src/x", "queue_size": 1000}}},
    ]}
    with Dataflow(desc, launcher=launcher) as df:
        box = {}
        t = threading.Thread(target=lambda: box.update(dst=Node("dst", dataflow=df.shm, device=0)))
        t.start()
        src = Node("src", dataflow=df.shm, device=0)
        t.join(60)
        dst = box["dst"]
        src.set_compact(compact)
        for seed in seeds:
            arr = ra.array(seed)
            _, info = ra.reference(arr, compact)
            with DeviceArray.from_pyarrow(arr) as da:
                src.send_output("x", da, {"seed": seed})
            ev = dst.next(timeout=30)
            assert ev is not None and ev["type"] == "INPUT", ev
            assert ev["metadata"]["seed"] == seed
            assert ev["data_len"] > 0, seed
            host = ev["value"].to_pyarrow()
            assert host.type == arr.type and host.equals(arr), (seed, host, arr)
            if compact:
                assert ra.mask_validity(ev["type_info"]) == ra.mask_validity(info), seed
                assert all(x["offset"] == 0 for x in ra.nodes(host)), seed
            else:
                assert ev["type_info"].to_json() == info.to_json(), seed
            del ev
        src.close()
        dst.close()
        df.wait(30)
