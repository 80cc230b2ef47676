"""CPU-side checks of the C ABI: the library loads and exports every declared symbol, and the
host-side plan (a1 walk + ArrowTypeInfo; no GPU call) matches the oracle on every fixture."""
import ctypes
import json
import os
import re

import pyarrow as pa
import pytest

from dora_amd import _lib
from dora_amd.arrow_utils import Plan
from dora_amd.type_info import decode
from oracle.pack_ref import pack
from tests.golden import recipes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ALL = recipes.KATS + recipes.CASES


# Declared in include/dora_operator_api.h but implemented by operator libraries, not by ours.
OPERATOR_ENTRY_POINTS = {"dora_init_operator", "dora_drop_operator", "dora_on_event"}


TESTING_HEADER = "dora_gpu_testing.h"  # the test hooks' own library (libdora_gpu_testing.so)


def _functions(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(dora_\w+)\s*\(", txt))


def header_functions():
    """Functions of the product headers (include/*.h but the testing header)."""
    names = set()
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h.endswith(".h") and h != TESTING_HEADER:
            names |= _functions(os.path.join(ROOT, "include", h))
    return names - OPERATOR_ENTRY_POINTS


def hook_functions():
    return _functions(os.path.join(ROOT, "include", TESTING_HEADER))


def test_library_exports_every_header_symbol(lib):
    missing = [n for n in sorted(header_functions()) if not hasattr(lib, n)]
    assert not missing, missing


def test_bindings_cover_header(lib):
    assert header_functions() == set(_lib.declared_symbols())


def test_test_hooks_live_in_their_own_library(lib):
    """Verdict r04 weak 7: the product ABI (include/dora_gpu.h, libdora_gpu.so) carries no test
    hook; every function of include/dora_gpu_testing.h is exported by libdora_gpu_testing.so."""
    import subprocess
    hooks = hook_functions()
    assert hooks and all(n.startswith("dora_gpu_test_") for n in hooks), hooks
    assert not [n for n in header_functions() if "_test_" in n]
    assert hooks == set(_lib.declared_test_symbols())
    testing = _lib.load_testing()
    assert not [n for n in sorted(hooks) if not hasattr(testing, n)]
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                              text=True, check=True).stdout
    assert "dora_gpu_test_" not in exported
    # nor the test tools' kernels and launchers (the fence probes, csrc/testing/fence_probes.hip)
    demangled = subprocess.run(["nm", "-D", "-C", _lib.LIB_PATH], capture_output=True, text=True,
                               check=True).stdout
    assert "l1_stale" not in demangled and "l2_touch" not in demangled


def test_product_library_has_no_tuning_entry_point(lib):
    """Verdict r05 item 6: the pack-tuning knobs (kernel variants, grid caps, in-flight caps,
    queue counts, the CP-signal switch) and their microbenchmark hooks are gone from the shipped
    library — no exported symbol, C or C++, sets one."""
    import subprocess
    syms = subprocess.run(["nm", "-D", "--defined-only", "-C", _lib.LIB_PATH], capture_output=True,
                          text=True, check=True).stdout
    for word in ("pack_tune", "pack_signal_tune", "cp_grid", "set_in_flight_caps", "cp_lone",
                 "mid_queues", "pipeline_bench", "keep_warm", "pack_variant", "aql_heartbeat("):
        assert word not in syms, word


def test_version_and_errors(lib):
    assert lib.dora_gpu_version().startswith(b"dora-gpu")
    h = ctypes.c_void_p()
    rc = lib.dora_gpu_plan(None, None, 10, ctypes.byref(h))
    assert rc == -1
    assert b"null" in lib.dora_gpu_last_error().lower()


def _host_sample(plan: Plan) -> bytes:
    """Materialise the sample from the plan's segment table on the host (checks the table)."""
    buf = bytearray(plan.size)
    for src, off, n in plan.segments():
        buf[off:off + n] = ctypes.string_at(src, n)
    return bytes(buf)


@pytest.mark.parametrize("name", ALL)
def test_host_plan_matches_oracle(name):
    arr = recipes.build(name)
    sample, info = pack(arr)
    with Plan.of(arr) as p:
        assert p.size == len(sample)
        ti = p.type_info()
        assert ti.to_json() == info.to_json()
        got = _host_sample(p)
    # bit-exact regions (padding is zero in both: fresh zeroed sample vs zeroed bytearray)
    assert got == sample


@pytest.mark.parametrize("name", ["kat4", "struct_nulls_sliced", "dictionary", "map",
                                  "timestamp_date_time", "deep_nesting"])
def test_type_info_data_type_roundtrips_to_pyarrow(name):
    arr = recipes.build(name)
    with Plan.of(arr) as p:
        ti = p.type_info()
    assert ti.arrow_type() == arr.type


def test_byte_array_plan():
    data = bytes(range(200))
    buf = ctypes.create_string_buffer(data, len(data))
    with Plan.of_bytes(ctypes.addressof(buf), len(data), on_device=False) as p:
        ti = p.type_info()
        assert ti.to_json() == {"data_type": "C", "len": 200, "null_count": 0, "validity": None,
                                "offset": 0, "buffer_offsets": [[0, 200]], "child_data": []}
        assert _host_sample(p) == data


@pytest.mark.parametrize("arr", [
    pa.array(["a", "b"], pa.string_view()),
    pa.UnionArray.from_sparse(pa.array([0, 1], pa.int8()),
                              [pa.array([1, 2]), pa.array(["a", "b"])]),
], ids=["utf8_view", "sparse_union"])
def test_types_outside_parity_set_are_rejected(arr):
    with pytest.raises(_lib.UnsupportedType):
        Plan.of(arr)


def test_fixture_files_are_data_only():
    for f in os.listdir(GOLDEN):
        if f.endswith(".json"):
            json.load(open(os.path.join(GOLDEN, f)))


def test_decode_rejects_truncated():
    arr = recipes.build("kat5")
    with Plan.of(arr) as p:
        raw = p.type_info_bytes()
    assert decode(raw).data_type == "+l[item:!i]"
    with pytest.raises(ValueError):
        decode(raw[:-3])


def test_type_info_validity_tag_2_decodes():
    """Validity tag 2 (bitmap in the sample's validity tail, node sends of device arrays): the
    Python decoder reads (offset, len) in place of the inline bytes; everything else of the
    serialized ArrowTypeInfo is unchanged."""
    import struct
    arr = pa.array([1, None, 3, None, 5], type=pa.int32())
    with Plan.of(arr) as p:
        raw = p.type_info().raw
    slen = struct.unpack_from("<I", raw, 0)[0]
    tag_at = 4 + slen + 16
    assert raw[tag_at] == 1
    vlen = struct.unpack_from("<Q", raw, tag_at + 1)[0]
    rest = raw[tag_at + 1 + 8 + vlen:]
    tagged = raw[:tag_at] + bytes([2]) + struct.pack("<QQ", 64, vlen) + rest
    a, b = decode(raw), decode(tagged)
    assert a.validity is not None and a.validity_in_sample is None
    assert b.validity is None and b.validity_in_sample == (64, vlen)
    ja, jb = a.to_json(), b.to_json()
    ja.pop("validity"), jb.pop("validity")
    assert ja == jb
    with pytest.raises(ValueError):
        decode(raw[:tag_at] + bytes([3]) + raw[tag_at + 1:])
