"""The strided views the gather is checked on, shared by its host emulation
(test_gather_index_host.py) and its GPU tests (test_gpu_tensor_device.py): the smallest that reach
each edge of a tile of 16, 32 or 64, odd sizes, every element size, negative and zero strides,
8 dimensions, outputs with no whole 16-byte unit, and the two frame-sized views of the probe."""
import numpy as np


def base(dtype, shape):
    """Distinct-looking values of `dtype` in row-major order (cheap for frame-sized arrays)."""
    n = int(np.prod(shape))
    return ((np.arange(n, dtype=np.int64) * 37 + 11) % 2039).astype(dtype).reshape(shape)  # exact in float16


# name -> (dtype, base shape, view of the base)
VIEWS = {
    "f32_67x129_T": (np.float32, (67, 129), lambda b: b.T),
    "u8_129x65_T": (np.uint8, (129, 65), lambda b: b.T),
    "f64_63x64_T": (np.float64, (63, 64), lambda b: b.T),
    "u8_hwc_to_chw_37x53x3": (np.uint8, (37, 53, 3), lambda b: b.transpose(2, 0, 1)),
    "f16_nchw_to_nhwc": (np.float16, (2, 5, 33, 65), lambda b: b.transpose(0, 2, 3, 1)),
    "u8_crop": (np.uint8, (130, 200), lambda b: b[3:120, 5:190]),
    "f32_drop_first_column": (np.float32, (64, 64), lambda b: b[:, 1:]),
    "i16_reversed_step2": (np.int16, (40, 60), lambda b: b[::-1, ::2]),
    "f32_broadcast": (np.float32, (1, 257), lambda b: np.broadcast_to(b, (9, 257))),
    "f64_4d_transpose": (np.float64, (5, 6, 7, 8), lambda b: b.transpose(3, 1, 0, 2)),
    "u8_8d_reversed_axes": (np.uint8, (2, 2, 2, 2, 2, 2, 2, 3), lambda b: b.transpose(*range(7, -1, -1))),
    "u8_105_bytes": (np.uint8, (3, 5, 7), lambda b: b.transpose(2, 0, 1)),
    "u8_byte_offset_3": (np.uint8, (20, 30), lambda b: b.reshape(-1)[3:3 + 19 * 30].reshape(19, 30)[:, :29]),
    "u8_frame_hwc_to_chw": (np.uint8, (1080, 1920, 3), lambda b: b.transpose(2, 0, 1)),
    "f32_1100x1024_T": (np.float32, (1100, 1024), lambda b: b.T),
}


def make(name):
    """(base array, view) of VIEWS[name]."""
    dtype, shape, fn = VIEWS[name]
    b = base(dtype, shape)
    return b, fn(b)


def describe_view(b, v, ptr):
    """(shape, strides in elements, dtype, byte offset) of view `v` of base `b` as a tensor over
    memory at `ptr` holding b's bytes."""
    off = v.__array_interface__["data"][0] - b.__array_interface__["data"][0]
    return v.shape, [s // v.dtype.itemsize for s in v.strides], v.dtype, off


def misalignment(b):
    """How many bytes past a multiple of its element size base `b` starts (numpy's own allocations
    are aligned: 0 except for a base laid over a shifted buffer, tests/random_views.py)."""
    return b.__array_interface__["data"][0] % b.itemsize
