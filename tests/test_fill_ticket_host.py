"""The self-published sample path on the CPU (no GPU): the public device header compiles on its
own for gfx950, dora_fill_ticket has one layout in C, C++ and the ctypes mirror, and
dora_sample_fill_ticket refuses what only a device slot can do (a host-only dataflow: inline and
shared-memory samples, NULL and foreign samples)."""
import ctypes
import os
import shutil
import subprocess
from ctypes import byref, c_void_p

import pytest

from dora_amd import _lib
from dora_amd._lib import FillTicket
from dora_amd.arrow_utils import Plan
from tests.test_dataflow_host import InProcessDaemon, _start_nodes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

ERR_INVALID, ERR_UNSUPPORTED = -1, -4


def test_device_header_compiles_on_its_own(tmp_path):
    """examples/publish_kernel.hip (a user kernel of ~30 lines) with nothing but include/ on the
    include path: the header pulls in nothing from dora_amd/csrc."""
    src = os.path.join(ROOT, "examples", "publish_kernel.hip")
    obj = str(tmp_path / "publish_kernel.o")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-c", "-I", INCLUDE, src, "-o", obj],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert os.path.getsize(obj) > 0
    for h in ("dora_gpu_device.h", "dora_fill_ticket.h"):
        text = open(os.path.join(INCLUDE, h)).read()
        assert "csrc" not in text and "pack_device" not in text, h


LAYOUT_SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "dora_gpu.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(dora_fill_ticket), offsetof(dora_fill_ticket, flag),
         offsetof(dora_fill_ticket, done), offsetof(dora_fill_ticket, epoch),
         offsetof(dora_fill_ticket, workgroups), offsetof(dora_fill_ticket, mode));
  return 0;
}
"""


@pytest.mark.parametrize("lang,ext,std", [("c", ".c", "-std=c11"), ("c++", ".cpp", "-std=c++17")])
def test_ticket_layout_matches_the_ctypes_mirror(tmp_path, lang, ext, std):
    """sizeof and every field offset as a C and as a C++ host compiler see them (through
    dora_gpu.h, which host code includes) equal the ctypes mirror's."""
    cc = shutil.which("cc" if lang == "c" else "c++") or HIPCC
    src = tmp_path / ("layout" + ext)
    src.write_text(LAYOUT_SNIPPET)
    exe = str(tmp_path / "layout")
    subprocess.run([cc, "-x", lang, std, "-I", INCLUDE, str(src), "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True,
                                          check=True).stdout.split()]
    want = [ctypes.sizeof(FillTicket)] + [getattr(FillTicket, f).offset for f in
                                          ("flag", "done", "epoch", "workgroups", "mode")]
    assert got == want == [32, 0, 8, 16, 24, 28]
    text = open(os.path.join(INCLUDE, "dora_fill_ticket.h")).read()
    assert "static_assert(sizeof(dora_fill_ticket) == DORA_FILL_TICKET_SIZE" in text


def _ticket(lib, node, sample, workgroups=4, mode=_lib.FILL_WRITE_THROUGH):
    t = FillTicket()
    rc = lib.dora_sample_fill_ticket(node, sample, workgroups, mode, byref(t))
    return rc, lib.dora_gpu_last_error().decode()


def test_host_only_node_refuses_tickets():
    """A node without a GPU: its samples are an inline Vec below 4096 B and a shared-memory region
    from there, both written by the host — no kernel can publish them.  The refusals name their
    reason, change nothing (the samples still send and arrive), and a NULL or foreign sample is
    an invalid argument."""
    lib = _lib.load()
    d = InProcessDaemon({"nodes": [
        {"id": "src", "outputs": ["out"]},
        {"id": "dst", "inputs": {"in": {"source": "src/out", "queue_size": 10}}, "outputs": []},
    ]})
    nodes = _start_nodes(d.shm, ["src", "dst"])
    tx, rx = nodes["src"], nodes["dst"]
    try:
        shm, inl = c_void_p(), c_void_p()
        _lib.call("dora_node_allocate_data_sample", tx.handle, 8192, byref(shm))
        _lib.call("dora_node_allocate_data_sample", tx.handle, 100, byref(inl))
        rc, msg = _ticket(lib, tx.handle, shm)
        assert rc == ERR_UNSUPPORTED and "shared-memory" in msg, (rc, msg)
        rc, msg = _ticket(lib, tx.handle, inl)
        assert rc == ERR_UNSUPPORTED and "inline" in msg, (rc, msg)
        rc, msg = _ticket(lib, tx.handle, None)
        assert rc == ERR_INVALID and "NULL" in msg, (rc, msg)
        # a sample of another node, and a pointer that is no sample at all
        foreign = c_void_p()
        _lib.call("dora_node_allocate_data_sample", rx.handle, 8192, byref(foreign))
        rc, msg = _ticket(lib, tx.handle, foreign)
        assert rc == ERR_INVALID and "not live on this node" in msg, (rc, msg)
        junk = ctypes.create_string_buffer(256)
        rc, msg = _ticket(lib, tx.handle, ctypes.cast(junk, c_void_p))
        assert rc == ERR_INVALID and "not live on this node" in msg, (rc, msg)
        lib.dora_sample_discard(rx.handle, foreign)
        # argument checks come before the slot's kind
        for wgs in (0, 4097):
            rc, msg = _ticket(lib, tx.handle, shm, workgroups=wgs)
            assert rc == ERR_INVALID and "workgroups" in msg, (wgs, rc, msg)
        rc, msg = _ticket(lib, tx.handle, shm, mode=7)
        assert rc == ERR_INVALID and "mode" in msg, (rc, msg)
        with pytest.raises(_lib.UnsupportedType):
            tx.sample_fill_ticket(shm, 1)
        # the refused samples are untouched: written by the host, sent, received
        ctypes.memset(lib.dora_sample_data(shm), 0x5A, 8192)
        ctypes.memset(lib.dora_sample_data(inl), 0x3C, 100)
        for smp, n in ((shm, 8192), (inl, 100)):
            with Plan.of_bytes(lib.dora_sample_data(smp), n, False) as p:
                ti = p.type_info_bytes()  # ArrowTypeInfo::byte_array(n)
            _lib.call("dora_node_send_output_sample", tx.handle, b"out", ti, len(ti), b"", 0, smp)
        for n, byte in ((8192, 0x5A), (100, 0x3C)):
            ev = rx.next(timeout=10)
            assert ev["type"] == "INPUT" and ev["data_len"] == n
            assert ctypes.string_at(ev["data_ptr"], n) == bytes([byte]) * n
            del ev
        # a sent sample is no longer live
        rc, msg = _ticket(lib, tx.handle, shm)
        assert rc == ERR_INVALID and "not live on this node" in msg, (rc, msg)
        so, sp = ctypes.c_uint64(9), ctypes.c_uint64(9)
        _lib.call("dora_node_sample_paths", tx.handle, byref(so), byref(sp))
        assert (so.value, sp.value) == (0, 0)
    finally:
        tx.close()
        rx.close()
        d.join()
