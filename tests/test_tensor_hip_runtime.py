"""One HIP runtime for a device tensor's producer and the node (no GPU needed: loading the
libraries initialises nothing).  torch's ROCm wheel carries its own libamdhip64: imported before
dora_amd, the library binds to it and the process holds one runtime; the other way round it
holds two, whose streams and allocation tables do not know each other, and the node refuses a
device tensor by name before it hands its stream to the producer.  Each order runs in a fresh
interpreter, since the outcome is a property of the process."""
import os
import subprocess
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = """
import os, sys
sys.path.insert(0, {root!r})
{first}
{second}
from dora_amd import _lib, node
_lib.load()
libs = {{os.path.realpath(l.rsplit(None, 1)[-1]) for l in open('/proc/self/maps')
        if os.path.basename(l.rsplit(None, 1)[-1]).startswith('libamdhip64')}}
try:
    node._require_one_hip_runtime()
    print('accepted', len(libs))
except RuntimeError as e:
    assert 'two HIP runtimes' in str(e) and 'Import' in str(e), str(e)
    print('refused', len(libs))
"""


def _run(first, second):
    r = subprocess.run([sys.executable, "-c", PROBE.format(root=ROOT, first=first, second=second)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    verdict, count = r.stdout.split()[-2:]
    return verdict, int(count)


def test_torch_imported_first_shares_one_runtime(lib):
    import torch  # noqa: F401
    assert _run("import torch", "import dora_amd.node") == ("accepted", 1)


def test_library_loaded_first_is_refused_when_torch_brings_its_own(lib):
    import torch
    own = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    verdict, count = _run("from dora_amd import _lib; _lib.load()", "import torch")
    if os.path.exists(own) and os.path.realpath(own) != os.path.realpath("/opt/rocm/lib/libamdhip64.so"):
        assert (verdict, count) == ("refused", 2)
    else:  # a torch built against the system's runtime: one either way
        assert (verdict, count) == ("accepted", 1)
