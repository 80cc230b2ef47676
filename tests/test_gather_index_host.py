"""The strided gather's address arithmetic on the CPU (no GPU): csrc/testing/gather_emulate.cpp, a
stand-alone program built here with the host compiler under AddressSanitizer and UBSan, runs the
function every lane of gather_rows_kernel runs (csrc/gather_device.h) for every lane of the grid,
over the descriptor dora_gpu_plan_tensor gives for each view the GPU tests use.  It fails unless
(a) every source offset lies in the plan's [lo, hi], (c) every output byte of [0, total) is
written exactly once and none outside; (d) the bytes it writes are compared here with numpy's
row-major copy of the view.  ((b), LDS indices: the kernel has no LDS phase.)  Views whose
strides put offsets beyond 2^32 run with addresses only."""
import os
import shutil
import subprocess
from ctypes import byref, c_int, c_int64, c_uint32, c_uint64, c_void_p

import numpy as np
import pytest

from dora_amd import _lib, tensor
from dora_amd._lib import ARROW_DEVICE_ROCM, DoraGpuError
from tests import gather_views

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x7F12_3456_0000  # a made-up device address, 16-byte aligned: planning never reads it
BIG = {"u8_frame_hwc_to_chw", "f32_1100x1024_T"}


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    if not cxx:
        pytest.fail("no host C++ compiler to build the gather emulation with")
    exe = str(tmp_path_factory.mktemp("gather") / "gather_emulate")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dora_amd", "csrc"),
           os.path.join(ROOT, "dora_amd", "csrc", "testing", "gather_emulate.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def gather_desc(ptr, shape, strides, dtype, byte_offset=0):
    """The plan's gather descriptor of a device tensor over `ptr`: dict, or None if dense."""
    t, keep = tensor._describe(ptr, shape, strides, dtype, byte_offset)
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor", byref(t), ARROW_DEVICE_ROCM, byref(h))
    try:
        g, src, nd, row, elem = c_int(), c_void_p(), c_int(), c_uint64(), c_uint32()
        shp, std = (c_int64 * 8)(), (c_int64 * 8)()
        lo, hi = c_int64(), c_int64()
        _lib.call("dora_gpu_test_plan_gather", h, byref(g), byref(src), byref(nd), byref(row),
                  byref(elem), shp, std, byref(lo), byref(hi))
        size = _lib.load().dora_gpu_plan_size(h)
    finally:
        _lib.load().dora_gpu_plan_free(h)
    if not g.value:
        return None
    return {"src": src.value, "nd": nd.value, "row": row.value, "elem": elem.value,
            "shape": list(shp)[:nd.value], "stride": list(std)[:nd.value], "lo": lo.value,
            "hi": hi.value, "total": size}


def run(exe, d, dst_addr, files=(), tile=False):
    cmd = [exe, *(["--tile"] if tile else []), d["elem"], d["row"], d["total"], d["lo"], d["hi"], d["src"], dst_addr, d["nd"],
           *d["shape"], *d["stride"], *files]
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith(("ok", "n/a") if tile else "ok"), \
        (r.stdout + r.stderr)[-2000:]
    return r.stdout


@pytest.mark.parametrize("name", list(gather_views.VIEWS))
def test_emulated_grid(lib, emulator, tmp_path, name):
    b, v = gather_views.make(name)
    shape, strides, dtype, off = gather_views.describe_view(b, v, FAKE)
    d = gather_desc(FAKE, shape, strides, dtype, off)
    assert d is not None and d["src"] == FAKE + off
    # the plan's interval is exactly the bytes of the base the view can reach
    raw = b.tobytes()
    assert 0 <= off + d["lo"] and off + d["hi"] < len(raw)
    src_file, out_file = str(tmp_path / "src.bin"), str(tmp_path / "out.bin")
    with open(src_file, "wb") as f:
        f.write(raw[off + d["lo"]: off + d["hi"] + 1])
    want = np.ascontiguousarray(v).tobytes()
    assert d["total"] == len(want)
    # an aligned destination; one 3 bytes off (a head, units that start mid-element) and one
    # 8 off for the small views
    for dst in (0x7F00_0000_1000,) + (() if name in BIG else (0x7F00_0000_1003, 0x7F00_0000_2008)):
        run(emulator, d, dst, (src_file, out_file))
        with open(out_file, "rb") as f:
            assert f.read() == want, (name, hex(dst))


# views gather_tile_kernel applies to at an element-aligned destination (a source-contiguous
# dimension that is not the output's innermost one); the others print "n/a"
TILED = {"f32_67x129_T", "u8_129x65_T", "f64_63x64_T", "u8_hwc_to_chw_37x53x3", "f16_nchw_to_nhwc",
         "f64_4d_transpose", "u8_8d_reversed_axes", "u8_105_bytes", "u8_frame_hwc_to_chw",
         "f32_1100x1024_T"}


@pytest.mark.parametrize("name", list(gather_views.VIEWS))
def test_emulated_tile_grid(lib, emulator, tmp_path, name):
    """gather_tile_kernel's phases over every view: (a)-(d), LDS indices included."""
    b, v = gather_views.make(name)
    shape, strides, dtype, off = gather_views.describe_view(b, v, FAKE)
    d = gather_desc(FAKE, shape, strides, dtype, off)
    raw = b.tobytes()
    src_file, out_file = str(tmp_path / "src.bin"), str(tmp_path / "out.bin")
    with open(src_file, "wb") as f:
        f.write(raw[off + d["lo"]: off + d["hi"] + 1])
    want = np.ascontiguousarray(v).tobytes()
    out = run(emulator, d, 0x7F00_0000_1000, (src_file, out_file), tile=True)
    assert out.startswith("ok") == (name in TILED), (name, out)
    if name in TILED:
        with open(out_file, "rb") as f:
            assert f.read() == want, name
    # a destination that is not element-aligned is never tiled
    if np.dtype(dtype).itemsize > 1:
        assert run(emulator, d, 0x7F00_0000_1003, tile=True).startswith("n/a")


def test_tile_addresses_beyond_32_bits(lib, emulator):
    """A transpose whose strides put source offsets past 2^32 (addresses only), and a row-like
    view the tile kernel must decline."""
    d = gather_desc(FAKE, (70, 5, 40), (1, 2 ** 33, 2 ** 20 + 4), np.float32)
    assert d["hi"] > 2 ** 32
    assert run(emulator, d, 0x7F00_0000_1000, tile=True).startswith("ok")
    d = gather_desc(FAKE, (4300, 64), (2 ** 20 + 3, 1), np.uint8)
    assert run(emulator, d, 0x7F00_0000_1000, tile=True).startswith("n/a")


def test_tiny_views(lib, emulator, tmp_path):
    """Outputs shorter than a unit, one element included."""
    for dtype, bshape, fn in [(np.uint8, (3, 2), lambda b: b.T), (np.float64, (2, 3), lambda b: b[:, 1:2]),
                              (np.float32, (2, 2), lambda b: b[1:, 1:])]:
        b = gather_views.base(dtype, bshape)
        v = fn(b)
        shape, strides, dt, off = gather_views.describe_view(b, v, FAKE)
        d = gather_desc(FAKE, shape, strides, dt, off)
        if d is None:  # a (1, 1) view is dense: one element, read in place
            assert v.size == 1
            continue
        src_file, out_file = str(tmp_path / "s.bin"), str(tmp_path / "o.bin")
        with open(src_file, "wb") as f:
            f.write(b.tobytes()[off + d["lo"]: off + d["hi"] + 1])
        for dst in (0x1000, 0x100F, 0x1001):
            run(emulator, d, dst, (src_file, out_file))
            with open(out_file, "rb") as f:
                assert f.read() == np.ascontiguousarray(v).tobytes()


BEYOND = {  # shape, strides in elements, dtype: offsets past 2^32, addresses only
    "row_stride_2^20+3_spanning_4GiB": ((4300, 64), (2 ** 20 + 3, 1), np.uint8),
    "both_strides_past_2^32": ((3, 5), (2 ** 33 + 1, 2 ** 32 + 7), np.uint8),
    "negative_past_2^32": ((5, 7, 4), (-(2 ** 34), 2 ** 32 + 2, 1), np.float32),
    "rows_past_2^32_odd_alignment": ((3, 100), (2 ** 33 + 5, 1), np.uint8),
}


@pytest.mark.parametrize("name", list(BEYOND))
def test_addresses_beyond_32_bits(lib, emulator, name):
    shape, strides, dtype = BEYOND[name]
    d = gather_desc(FAKE, shape, strides, dtype)
    item = np.dtype(dtype).itemsize
    lo = sum((n - 1) * s * item for n, s in zip(shape, strides) if s < 0)
    hi = sum((n - 1) * s * item for n, s in zip(shape, strides) if s > 0) + item - 1
    assert (d["lo"], d["hi"]) == (lo, hi) and hi - lo > 2 ** 32
    for dst in (0x7F00_0000_1000, 0x7F00_0000_1005):
        run(emulator, d, dst)


def test_the_emulation_notices_a_reach_one_byte_short(lib, emulator):
    """The checks bite: with the interval cut by one byte at either end the same run fails."""
    b, v = gather_views.make("i16_reversed_step2")
    shape, strides, dtype, off = gather_views.describe_view(b, v, FAKE)
    d = gather_desc(FAKE, shape, strides, dtype, off)
    run(emulator, d, 0x1000)
    for key, delta in (("hi", -1), ("lo", 1)):
        cut = dict(d, **{key: d[key] + delta})
        cmd = [emulator, cut["elem"], cut["row"], cut["total"], cut["lo"], cut["hi"], cut["src"],
               0x1000, cut["nd"], *cut["shape"], *cut["stride"]]
        r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout.startswith("FAIL"), (key, r.stdout, r.stderr[-500:])


def test_nine_dimensions_are_refused(lib):
    with pytest.raises(DoraGpuError) as e:
        gather_desc(FAKE, (4,) * 9, [2 * 8 ** k for k in range(8, -1, -1)], np.uint8)
    assert e.value.code == -4
