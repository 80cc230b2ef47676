"""What dora_amd._dora_node.send_tensor_crops does with its DLPack capsules, as
tests/test_pyext_capsules_host.py holds the other send functions to it: the boxes' capsule joins
the fields' — every capsule of a well-formed call is consumed (renamed "used_dltensor", its deleter
run exactly once), and a call refused for its arguments leaves every capsule untouched.

No GPU and no node: the send goes to handle None, which the C entry refuses with DORA_ERR_INVALID
before it does anything, so the whole marshalling runs and nothing is sent."""
import gc
import sys
import weakref

import numpy as np
import pytest

from dora_amd import _dora_node as fast
from tests.test_pyext_capsules_host import CPU, NAMED, NOT_A_CAPSULE, _capsules, _untouched, _values, _name

USAGE = ("send_tensor_crops(handle, output_id, names, capsules, crops, device_type, metadata, "
         "flags)" + NAMED + "; crops a tuple as long, of None or (mode, axis0, axis1, size0, size1, "
         "code, bits, boxes)")
ENTRY = (2, 0, 1, 4, 5, 2, 32)  # bilinear, axes (0, 1) to (4, 5), float32


def _boxes():
    return np.array([[0, 0, 2, 3], [1, 1, 2, 2]], dtype=np.int32)


def args(caps, boxes, names=("a", "b"), entries=None):
    entries = (ENTRY + (boxes[0],), ENTRY + (boxes[1],)) if entries is None else entries
    return (None, "out", names, tuple(caps), entries, CPU, None, 0)


def refused(call, text, caps):
    with pytest.raises(TypeError) as e:
        fast.send_tensor_crops(*call)
    assert str(e.value) == text
    assert _untouched(*caps)


def test_a_well_formed_call_consumes_every_capsule_once():
    arrays = [_values(), _values(), _boxes(), _boxes()]
    before = [sys.getrefcount(a) for a in arrays]
    caps = _capsules(arrays)
    assert [sys.getrefcount(a) for a in arrays] == [n + 1 for n in before]
    rc = fast.send_tensor_crops(*args(caps[:2], caps[2:]))
    assert isinstance(rc, int) and rc != 0  # (no node: DORA_ERR_INVALID, nothing sent)
    assert all(_name(c) == b"used_dltensor" for c in caps)
    assert [sys.getrefcount(a) for a in arrays] == before  # every deleter has run, and once
    refs = [weakref.ref(a) for a in arrays]
    del arrays
    gc.collect()
    assert all(r() is None for r in refs)
    # a field without crops brings no boxes
    arrays = [_values(), _values(), _boxes()]
    caps = _capsules(arrays)
    rc = fast.send_tensor_crops(*args(caps[:2], None, entries=(None, ENTRY + (caps[2],))))
    assert rc != 0 and all(_name(c) == b"used_dltensor" for c in caps)


def test_refused_calls_leave_every_capsule_untouched():
    caps = _capsules([_values(), _values(), _boxes(), _boxes()])
    f, b = caps[:2], caps[2:]
    refused(args(f, [b[0], object()]), "field 1: the boxes: " + NOT_A_CAPSULE, caps)
    refused(args([f[0], object()], b), "field 1: " + NOT_A_CAPSULE, caps)
    refused(args(f, [f[0], b[1]]), "capsules 0 and 2 are one capsule", caps)
    refused(args(f, [b[0], b[0]]), "capsules 2 and 3 are one capsule", caps)
    refused(args([f[0], f[0]], b), "fields 0 and 1 share one capsule", caps)
    refused(args(f, b)[:-1], USAGE, caps)
    refused(args(f, b, entries=(ENTRY + (b[0],),)), USAGE, caps)
    refused(args(f, b, entries=(ENTRY, ENTRY + (b[1],))), USAGE, caps)
    refused(args(f, b, entries=((0,) + ENTRY[1:] + (b[0],), None)),
            "field 0: crops entry (mode 0, axes 0 and 1, code 2, 32 bits)", caps)
