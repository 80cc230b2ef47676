"""What dora_amd._dora_node does with the DLPack capsules of a tensor send: every capsule of a
well-formed call is consumed (renamed "used_dltensor", its deleter run exactly once), and a call
refused for its arguments leaves every capsule untouched.

No GPU and no node: every send goes to handle None, which each C entry refuses with
DORA_ERR_INVALID before it does anything, so the whole marshalling runs and nothing is sent."""
import ctypes
import gc
import sys
import weakref

import numpy as np
import pytest

from dora_amd import node as _node  # noqa: F401  (refuses a tree without the extension)
from dora_amd import _dora_node as fast

CPU = 1       # ARROW_DEVICE_CPU
LENGTHS = 0   # DORA_PARTITION_LENGTHS

_name = ctypes.pythonapi.PyCapsule_GetName
_name.restype = ctypes.c_char_p
_name.argtypes = [ctypes.py_object]

NAMED = ": names is None over one capsule or a tuple as long as the tuple of capsules"
USAGE = {
    "send_tensor": "send_tensor(handle, output_id, capsule, device_type, metadata, flags)",
    "send_tensor_struct": "send_tensor_struct(handle, output_id, names, capsules, device_type, "
                          "metadata, flags): names and capsules are tuples of one length",
    "send_tensor_cast": "send_tensor_cast(handle, output_id, names, capsules, casts, device_type, "
                        "metadata, flags)" + NAMED + "; casts a tuple as long, of None or (code, "
                        "bits, scale)",
    "send_tensor_convert": "send_tensor_convert(handle, output_id, names, capsules, entries, "
                           "device_type, metadata, flags)" + NAMED + "; entries a tuple as long, "
                           "of None, (code, bits, scale) or (code, bits, scale, zero_point)",
    "send_tensor_reduce": "send_tensor_reduce(handle, output_id, names, capsules, reduces, "
                          "device_type, metadata, flags)" + NAMED + "; reduces a tuple as long, "
                          "of None or (op, axis, code, bits)",
    "send_tensor_resize": "send_tensor_resize(handle, output_id, names, capsules, resizes, "
                          "device_type, metadata, flags)" + NAMED + "; resizes a tuple as long, "
                          "of None or (mode, axis0, axis1, size0, size1, code, bits)",
    "send_tensor_list": "send_tensor_list(handle, output_id, names, capsules, partition, form, "
                        "partition_device, device_type, metadata, flags)" + NAMED,
    "send_tensor_take": "send_tensor_take(handle, output_id, names, capsules, index, "
                        "index_device, partition, form, partition_device, device_type, metadata, "
                        "flags)" + NAMED,
    "send_tensor_masked": "send_tensor_masked(handle, output_id, names, capsules, mask, "
                          "mask_device, partition, form, partition_device, device_type, "
                          "metadata, flags)" + NAMED,
}
NOT_A_CAPSULE = "expected a DLPack capsule named \"dltensor\" (an unused, unversioned one)"
NOT_A_TABLE = "a table is a DLPack capsule named \"dltensor\" (an unused, unversioned one)"

F32, F16 = (2, 32), (2, 16)  # (DLPack type code, bits)
I8, I32 = (0, 8), (0, 32)


def _values():
    return np.arange(6, dtype=np.float32).reshape(2, 3)


def _words():
    return np.array([1, 1], dtype=np.int32)


def _table():
    return np.array([1.0, 2.0, 3.0], dtype=np.float32)


def _bools():
    return np.array([True, False])


class Send:
    """One send function of the extension over two fields `a` and `b` (send_tensor: one tensor):
    `entries`, its per-field entries; `aux`, a maker per capsule that travels beside the fields
    (each with the word a refusal calls it by); `call(names, caps, entries, aux)`, its
    arguments."""

    def __init__(self, key, call, entries=None, aux=(), fields=2, shared="fields 0 and 1 share "
                 "one capsule"):
        self.key, self.name = key, key.split("+")[0]
        self.fn = getattr(fast, self.name)
        self.call, self.entries, self.aux, self.fields = call, entries, aux, fields
        self.shared = shared
        self.usage = USAGE[self.name]

    def __repr__(self):
        return self.key

    def arrays(self):
        return [_values() for _ in range(self.fields)], [make() for _, make in self.aux]

    def args(self, caps, aux, names=("a", "b"), entries=None):
        return self.call(names, tuple(caps), self.entries if entries is None else entries, aux)


def _entry_call(names, caps, entries, aux):
    return (None, "out", names, caps, entries, CPU, None, 0)


def _affine_call(names, caps, entries, aux):
    # field a: a scale table along axis 1; field b: a bias table along axis 1 and a scalar bias
    return (None, "out", names, caps, entries, CPU, None, 0,
            ((aux[0], None, 1, None), (None, aux[1], 1, 0.5)))


def _selected_call(names, caps, entries, aux):
    return (None, "out", names, caps, aux[0], CPU, aux[1], LENGTHS, CPU, CPU, None, 0)


ONE = "capsules 0 and 1 are one capsule"
SENDS = [
    Send("send_tensor", lambda names, caps, e, aux: (None, "out", caps[0], CPU, None, 0), fields=1),
    Send("send_tensor_struct", lambda names, caps, e, aux: (None, "out", names, caps, CPU, None, 0)),
    Send("send_tensor_cast", _entry_call, entries=(F16 + (None,), None)),
    Send("send_tensor_convert", _entry_call, entries=(I8 + (0.5, 3), F16 + (2.0,))),
    Send("send_tensor_convert+affine", _affine_call, entries=(F16 + (None,), F32 + (None,)),
         aux=(("table", _table), ("table", _table))),
    Send("send_tensor_reduce", _entry_call, entries=((1, 1) + I32, None)),
    Send("send_tensor_resize", _entry_call, entries=((1, 0, 1, 4, 5) + F32, None)),
    Send("send_tensor_list",
         lambda names, caps, e, aux: (None, "out", names, caps, aux[0], LENGTHS, CPU, CPU, None, 0),
         aux=(("partition", _words),), shared=ONE),
    Send("send_tensor_take", _selected_call, aux=(("index", _words), ("partition", _words)),
         shared=ONE),
    Send("send_tensor_masked", _selected_call, aux=(("mask", _bools), ("partition", _words)),
         shared=ONE),
]
RECORDS = [s for s in SENDS if s.fields == 2]
WITH_ENTRIES = [s for s in SENDS if s.entries is not None]
WITH_AUX = [s for s in SENDS if s.aux]


def _capsules(arrays):
    return [a.__dlpack__() for a in arrays]


def _untouched(*caps):
    return all(_name(c) == b"dltensor" for c in caps)


def _refused(send, args, text, caps):
    with pytest.raises(TypeError) as e:
        send.fn(*args)
    assert str(e.value) == text
    assert _untouched(*caps)


@pytest.mark.parametrize("send", SENDS, ids=repr)
def test_a_well_formed_call_consumes_every_capsule_once(send):
    values, others = send.arrays()
    arrays = values + others
    before = [sys.getrefcount(a) for a in arrays]
    caps, aux = _capsules(values), _capsules(others)
    assert [sys.getrefcount(a) for a in arrays] == [n + 1 for n in before]
    rc = send.fn(*send.args(caps, aux))
    assert isinstance(rc, int) and rc != 0  # (no node: DORA_ERR_INVALID, nothing sent)
    assert all(_name(c) == b"used_dltensor" for c in caps + aux)
    # every deleter has run, and once: each producer is back to the references it had before
    # its capsule was made, with the capsules still alive, and is then collectable
    assert [sys.getrefcount(a) for a in arrays] == before
    refs = [weakref.ref(a) for a in arrays]
    del arrays, values, others
    gc.collect()
    assert all(r() is None for r in refs)
    del caps, aux
    gc.collect()


@pytest.mark.parametrize("send", SENDS, ids=repr)
def test_a_field_that_is_no_capsule(send):
    values, others = send.arrays()
    caps, aux = _capsules(values), _capsules(others)
    real = caps[:-1] + aux
    text = NOT_A_CAPSULE if send.fields == 1 else f"field {send.fields - 1}: " + NOT_A_CAPSULE
    _refused(send, send.args(caps[:-1] + [object()], aux), text, real)
    # a used capsule is no capsule to consume either
    used = _capsules([_values()])[0]
    assert fast.send_tensor(None, "out", used, CPU, None, 0) != 0 and not _untouched(used)
    _refused(send, send.args(caps[:-1] + [used], aux), text, real)


@pytest.mark.parametrize("send,which", [(s, i) for s in WITH_AUX for i in range(len(s.aux))],
                         ids=lambda v: repr(v))
def test_a_travelling_tensor_that_is_no_capsule(send, which):
    values, others = send.arrays()
    caps, aux = _capsules(values), _capsules(others)
    word = send.aux[which][0]
    text = f"field {which}: " + NOT_A_TABLE if word == "table" else f"{word}: " + NOT_A_CAPSULE
    broken = list(aux)
    broken[which] = object()
    _refused(send, send.args(caps, broken), text, caps + aux)


@pytest.mark.parametrize("send", RECORDS, ids=repr)
def test_two_fields_share_a_capsule(send):
    values, others = send.arrays()
    caps, aux = _capsules(values), _capsules(others)
    _refused(send, send.args([caps[0], caps[0]], aux), send.shared, caps + aux)


@pytest.mark.parametrize("send", WITH_AUX, ids=repr)
def test_a_travelling_tensor_shares_a_capsule(send):
    values, others = send.arrays()
    caps, aux = _capsules(values), _capsules(others)
    table = send.aux[0][0] == "table"
    # the first of them is field a's capsule
    text = "field 0: a table shares a field's capsule" if table else \
        "capsules 0 and 2 are one capsule"
    _refused(send, send.args(caps, [caps[0]] + aux[1:]), text, caps + aux)
    if len(aux) == 2:  # the second is the first
        text = "field 1: two tables share one capsule" if table else \
            "capsules 2 and 3 are one capsule"
        _refused(send, send.args(caps, [aux[0], aux[0]]), text, caps + aux)


@pytest.mark.parametrize("send", SENDS, ids=repr)
def test_the_usage_string(send):
    values, others = send.arrays()
    caps, aux = _capsules(values), _capsules(others)
    # an argument short (the affine entries are the optional ninth: two short)
    args = send.args(caps, aux)
    _refused(send, args[:-2] if "+" in send.key else args[:-1], send.usage, caps + aux)
    if send.fields == 1:
        return
    _refused(send, send.args(caps, aux, names=("a", "b", "c")), send.usage, caps + aux)
    _refused(send, send.args(caps, aux, names=("a",)), send.usage, caps + aux)
    if send.name != "send_tensor_struct":  # (no names: one bare tensor)
        _refused(send, send.args(caps, aux, names=None), send.usage, caps + aux)


@pytest.mark.parametrize("send", WITH_ENTRIES, ids=repr)
def test_an_entry_tuple_of_the_wrong_length(send):
    values, others = send.arrays()
    caps, aux = _capsules(values), _capsules(others)
    short = (send.entries[0][:2], None)
    _refused(send, send.args(caps, aux, entries=short), send.usage, caps + aux)
    _refused(send, send.args(caps, aux, entries=send.entries[:1]), send.usage, caps + aux)
    long = (send.entries[0] + (0,) * 5, None)
    _refused(send, send.args(caps, aux, entries=long), send.usage, caps + aux)


def test_an_affine_entry_of_the_wrong_length():
    send = next(s for s in SENDS if s.key == "send_tensor_convert+affine")
    values, others = send.arrays()
    caps, aux = _capsules(values), _capsules(others)
    args = send.args(caps, aux)
    _refused(send, args[:-1] + (((aux[0], None, 1), None),),
             "field 0: an affine entry is None or (scale table, bias table, axis, bias)",
             caps + aux)
    _refused(send, args[:-1] + (args[-1][:1],), send.usage, caps + aux)
