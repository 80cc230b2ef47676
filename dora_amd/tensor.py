"""Tensors as messages.

A tensor of shape `(d0, d1, .., dk)` and dtype `T` travels as the Arrow array of length `d0` and
type `FixedSizeList<..FixedSizeList<T>[dk]..>[d1]` built from its row-major values (child fields
named `item`, nullable, as pyarrow creates them); a 1-D tensor is the plain primitive array.  Its
sample is one buffer, the row-major bytes, so the shape travels in the type and a node of the
reference can send or receive the same message.

    node.send_output("image", frame.transpose(2, 0, 1))   # numpy or CPU torch: any host DLPack tensor
    node.send_output("image", frame_cuda.permute(2, 0, 1))  # a torch tensor in this node's HBM
    chw = tensor.to_torch(event["value"])                  # device receiver: zero-copy, in HBM
    chw = tensor.to_numpy(event["value"])                  # host receiver: the nested pyarrow array
    chw = tensor.to_numpy(event["value"].to_pyarrow())     # device receiver: downloaded first

A record of tensors that share their leading extent travels as one message, the Arrow array of
type `Struct<name: T, ..>` whose fields are those tensor columns (nullable, as
`pa.StructArray.from_arrays` makes them); tensors of unrelated shapes get a leading extent of 1
(`unsqueeze(0)`), a struct of length 1:

    node.send_output("det", {"bbox": out[:, :4], "conf": out[:, 4], "cls": out[:, 5]})
    det = tensor.to_torch(event["value"])                  # {"bbox": .., "conf": .., "cls": ..}

A ragged batch — N rows of a tensor, or of a dict of tensors sharing N, cut into B lists of
different lengths — travels as one message too, the Arrow array of length B and type
`List<item: T>` (int32 offsets; `T` the tensor's or the record's type above):

    node.send_output("clouds", tensor.ragged({"x": p[:, 0], "y": p[:, 1]}, lengths=counts))
    node.send_output("dets", tensor.ragged(out[:, :4], offsets=nt.offsets()))  # offsets in HBM
    r = tensor.to_torch(event["value"])                    # Ragged: r.values, r.offsets (int32)

A partition on the host (a sequence, numpy, a CPU tensor) is checked inside the send: lengths are
non-negative and sum to N, offsets start at 0, never decrease and end at N, else the send raises
and nothing leaves.  A partition in this node's HBM (device values only) is never read on the
host: the send's one kernel launch turns it into offsets, clamped so that the message is a
well-formed List whatever the words hold — a partition that does not describe N rows is then the
producer's bug and shows as other list boundaries, not as an error.

Selected rows — what NMS, a score threshold or top-k end in — travel without the indexed copy:
`take(values, index)` stands for `values[index]` along dimension 0 (`values` a tensor or a dict
of tensors sharing N, `index` K int32 or int64 row numbers, repeats allowed) and is sent as
exactly the message `values[index]` would be, a tensor, a struct or, under `ragged`, a List whose
partition describes the K taken rows:

    node.send_output("det", tensor.take({"bbox": out[:, :4], "conf": out[:, 4]}, keep))
    node.send_output("det", tensor.ragged(tensor.take(fields, keep), lengths=per_image_counts))

The index lives where the values live.  A host index is checked inside the send: a word outside
[0, N) raises (no negative wrap-around) and nothing leaves.  An index in this node's HBM is never
read on the host: the send's one kernel launch reads row `index[i]` of every field straight into
the sample, no intermediate tensor and no synchronisation, and writes a row of zeros where a word
is not a row — a bad index is the producer's bug and shows as zero rows, never as a malformed
message or a stray read.  Not offered: other dimensions, a host index over device values.

Rows selected by a mask — what a score threshold, a point-cloud crop or a range filter produce —
travel without `values[mask]` and without `nonzero`, both of which synchronise with the GPU:
`masked(values, mask)` (`values` a tensor or a dict of tensors sharing N, `mask` N bool or uint8
elements, any non-zero one selecting its row) is sent as a `List` message whose child keeps the
**capacity** of N rows — the K selected rows in source order in front, zero rows behind — and
whose offsets, written where the mask is, say how many are live: `[0, K]` on its own, `C[p]` under
`ragged`, whose partition `p` then describes the N *source* rows (`C[i]` counts the selected rows
before row i), because K is not known on the host:

    node.send_output("det", tensor.masked({"bbox": out[:, :4], "conf": out[:, 4]}, conf > 0.5))
    node.send_output("det", tensor.ragged(tensor.masked(fields, keep), lengths=candidates_per_image))
    r = tensor.to_torch(event["value"])    # Ragged: r.values has N rows, r.offsets[-1] == K live

The mask lives where the values live.  The wire form is the same either way — `from_numpy_masked`
states it — so a host producer that wants the tight message sends `values[mask]` itself.  A mask
in this node's HBM is never read on the host: two small gfx950 kernels compact it into an index
and running counts in scratch behind the sample, and the send's gather reads the rows through it.
Not offered: masks along other dimensions, a host mask over device values, a cast under a mask.

A tensor whose consumer wants another element type is converted inside the send:
`cast(x, dtype, scale=None)` stands for "`x` converted to `dtype`" (float16 or float32, from uint8,
int8, uint16, int16, float16, bfloat16 or float32) and is sent as exactly the message the converted
tensor would be, bare or as a field of a dict next to fields that are sent as they are:

    node.send_output("image", tensor.cast(frame.permute(2, 0, 1), "float16", scale=1 / 255))
    node.send_output("det", {"image": tensor.cast(img, "float16", scale=1 / 255), "conf": conf})
    node.send_output("logits", tensor.cast(bf16_logits, "float32"))   # the way to send bfloat16

Element by element the result is `to_dtype(float32(x) * float32(scale))`: one float32
multiplication and one round-to-nearest-even conversion, float16 subnormals kept, overflow to
inf — `from_numpy_cast` states it in numpy and the send is bit-exact against it except for the
payload of a NaN.  Multiplying by `1 / 255` is not dividing by 255: the two differ in the last bit
for some inputs.  Host tensors are converted by the CPU inside the send; tensors in this node's
HBM by the send's one kernel launch, which reads the source once and writes the sample once, no
`.to(dtype)` and no intermediate tensor.  Not offered: a cast under `ragged` or `take`, bfloat16
destinations; integer destinations are `quantize`.

A tensor of float results that its consumers read as small integers — a mask or heat map in
[0, 1] as uint8 pixels, depth in metres as uint16 millimetres, activations as int8 — is quantised
inside the send: `quantize(x, dtype, scale=None, zero_point=0)` stands for "`x` quantised to
`dtype`" (uint8, int8, uint16 or int16, from the seven cast sources) and is sent as exactly the
message the quantised tensor would be, bare or as a value of a dict next to plain and `cast`
fields:

    node.send_output("mask", tensor.quantize(prob.permute(1, 2, 0), "uint8", scale=255))
    node.send_output("depth", tensor.quantize(metres, "uint16", scale=1000))
    node.send_output("out", {"mask": tensor.quantize(m, "uint8", 255), "feat": tensor.cast(f, "float32")})

Element by element, `[lo, hi]` the range of `dtype`: `y = float32(x) * float32(scale)` (one
float32 multiplication), `r = rint(y)` (ties to even), a NaN counts as 0, and
`q = int32(clip(r, lo - zero_point, hi - zero_point)) + zero_point`, so infinities and anything out
of range saturate.  `zero_point` is an integer in `[lo, hi]`.  `from_numpy_quantize` states it in
numpy and every send, from host and from device, is bit-exact against it for every input.  In
place of `x.mul(255).round().clamp(0, 255).to(torch.uint8)` and its launches and intermediates
the send's one launch reads the source once and writes a sample a half or a quarter the size.
Not offered: a quantise under `ragged`, `take` or `masked`; per-channel zero points.

Both take a bias and per-channel values, which is what normalisation and per-channel quantisation
need: `cast(x, dtype, scale=None, *, bias=None, axis=None)` and `quantize(x, dtype, scale=None,
zero_point=0, *, bias=None, axis=None)`, `scale` and `bias` each one number or a 1-D table of one
value per channel along `axis`, a dimension of `x` as given (after any `permute`; negative: from
the back):

    s, b = 1 / (255 * std), -mean / std                    # (x / 255 - mean[c]) / std[c] = x * s[c] + b[c]
    node.send_output("image", tensor.cast(frame.permute(2, 0, 1), "float16", scale=s, bias=b, axis=0))
    node.send_output("act", tensor.quantize(feat, "int8", scale=per_channel, axis=1))
    node.send_output("out", {"image": tensor.cast(img, "float16", scale=s, bias=b, axis=-1), "conf": conf})

With C the extent of `axis` and `inner` the product of the extents behind it, output element `e`
(row-major) has channel `c = (e / inner) % C` and `y = float32(x) * S + B`: two float32
operations, the product rounded and then the sum, never one fused multiply-add; `S` is
`scale[c]`, the scalar scale or absent (no multiplication), `B` is `bias[c]`, the scalar bias or
absent (no addition, so a zero product keeps its sign).  Then the cast or the quantise as above.
`from_numpy_cast` and `from_numpy_quantize` state it in numpy with `bias=` and `axis=`, and every
send is bit-exact against them but for a NaN's payload in a float destination.  A scalar and a
table may be mixed; a table needs `axis`, and `axis` needs a table.  Tables live where the values
live.  With host values a table is a sequence, a numpy array or a CPU tensor, converted to float32
and checked inside the send: length C, every value finite, else the send raises and nothing
leaves.  With values in this node's HBM a table is a float32 tensor in this node's HBM, 1-D, dense,
of C elements; it is never read on the host, so whatever it holds the result is the formula (a
NaN or an infinity propagates, and under a quantise saturates or becomes `zero_point`), and no
word outside the table is read.  A host table over device values raises: make the table once on
the device.  Not offered: per-channel zero points, a host table over device values, a conversion
under `ragged`, `take` or `masked`, bfloat16 destinations.

A class map — what a segmentation head or a classifier ends in — is reduced inside the send:
`argmax(x, axis, dtype="int64")` stands for "the index of the maximum of `x` along `axis`" (`x` a
tensor of one of the seven cast sources with at least two dimensions, any strided view; `axis` a
dimension of `x` as given, after any `permute`, negative: from the back; `dtype` uint8, uint16,
int32 or int64) and is sent as exactly the message the index tensor would be, `x`'s shape without
`axis`, bare or as a value of a dict next to plain fields and other `argmax` fields, which share
the leading extent of their *output* shapes:

    node.send_output("cls", tensor.argmax(logits, 0, "uint8"))            # (C, H, W) -> (H, W)
    node.send_output("top1", tensor.argmax(bf16_logits, -1, "int32"))     # (B, 1000) -> (B,)
    node.send_output("out", {"cls": tensor.argmax(seg, 1, "uint8"), "depth": depth[:, ::2]})

For each output element with candidates `v[0..C)` in view order the result is the smallest `c`
such that `v[c]` is a NaN, or without a NaN the smallest `c` with `v[c] >= v[k]` for all `k`:
numpy's and torch's rule, `-0.0` and `+0.0` tie.  Nothing is rounded, so every send, from host
memory or HBM, equals `from_numpy_argmax` exactly.  In place of `logits.argmax(0).to(torch.uint8)`
with its reduction launch, 8-byte indices, cast launch and two intermediates, the send's one launch
reads the logits once and writes only the message; it takes bfloat16 logits, which no plain send
accepts.  Refused, nothing leaving the node: fewer than two dimensions, an axis outside them, an
axis of extent 0, an extent whose last index does not fit `dtype` (uint8 with C > 256, ..), another
source or index dtype.  Not offered: `argmin`, the maximum's value, a reduction beside a conversion
in one dict, a reduction under `ragged`, `take` or `masked`, more than one axis.

A resized frame — what every vision dataflow starts with — is resized inside the send:
`resize(x, size, axes=(-2, -1), mode="nearest", dtype=None)` stands for "`x` with the two
dimensions `axes` at the new extents `size`" (`x` a tensor of one of the seven cast sources with 2
to 8 dimensions, any strided view; `axes` two different dimensions of `x` as given, after any
`permute`, negative: from the back; `mode` "nearest" or "bilinear"; `dtype` float16, float32,
uint8, int8, uint16 or int16, by default the source's own, which a bfloat16 source cannot keep) and
is sent as exactly the message the resized tensor would be, bare or as a value of a dict next to
plain fields and other `resize` fields, which share the leading extent of their *output* shapes:

    node.send_output("image", tensor.resize(frame, (640, 640), axes=(0, 1), mode="bilinear"))
    node.send_output("image", tensor.resize(frame.permute(2, 0, 1), (320, 320), mode="bilinear",
                                            dtype="float16"))
    node.send_output("out", {"thumb": tensor.resize(frames, (90, 160), axes=(1, 2)), "stamp": t})

An axis of source extent I and output extent O, both 1 to 32768, reads at output coordinate o the
tap `(o * I) // O` (nearest: OpenCV's INTER_NEAREST, torch's "nearest") or, bilinear with
half-pixel centres and no antialiasing, with `d = 2 * O`, `n = max((2 * o + 1) * I - O, 0)` and
`q = n // d`, the taps `q` and `q + 1` with weights `float32(d - n % d) / float32(d)` and
`float32(n % d) / float32(d)`, or the last element alone where `q >= I - 1`.  Every source element
is widened to float32; the four taps are blended along the second of `axes`, then along the first,
every product rounded to float32 and then every sum, never fused; the result is rounded to `dtype`
as `cast` does (floats) or as `quantize` does without a scale (integers: ties to even, saturated,
a NaN as 0).  Every send, from host memory or HBM, equals `from_numpy_resize` bit for bit but for
the payload of a NaN; torch's `interpolate` computes its weights from a float32 scale factor and
differs in the last bits.  In place of `permute`, `float()`, `interpolate`, `round`, `clamp`,
`to(uint8)`, `permute` and `contiguous` with their full-size intermediates, the send's one launch
reads only the taps it needs and writes only the small message.  Refused, nothing leaving the
node: fewer than two dimensions, an axis outside them, the two axes equal, an extent outside 1 to
32768, another source, destination or mode.  Not offered: bicubic, area and antialiased modes,
`align_corners=True`, one axis alone or more than two, a resize beside a conversion or an argmax
in one dict, a resize of or under `cast`, `quantize`, `argmax`, `ragged`, `take` or `masked`,
bfloat16 destinations.

A strided host view is gathered into row-major order by the CPU inside the send; pinned memory
is copied once, so every source has been read when `send_output` returns.  A tensor in device
memory is read by a kernel: in place when dense, gathered by the gfx950 gather kernel when it is a
strided view (one read and one write of HBM, no `.contiguous()` first).  The producer must share
the HIP runtime of this library: import torch before dora_amd (Node._send_tensor).

The hand-off from a detector to a second-stage model — K boxes cut out of one frame and brought to
one size — is done inside the send: `crops(frame, boxes, size, axes=(-2, -1), mode="bilinear",
dtype=None)` stands for the tensor of shape `(K,) + frame.shape` with the two extents at `axes`
replaced by `size`.  `boxes` is a dense `[K, 4]` int32 tensor next to the frame (host with host,
this node's HBM with HBM, where it is never read on the host), row k `(a_lo, b_lo, a_hi, b_hi)`:
half-open ranges along `axes[0]` and `axes[1]`.  Every coordinate is clamped to the frame on its
own; an empty or inverted box gives a crop of zeros; every other crop equals
`from_numpy_resize(frame[.., a0:a1, .., b0:b1, ..], size, ..)` bit for bit.  `mode` and `dtype` are
`resize`'s.  It is sent bare or as a value of a dict next to plain fields and other `crops`, which
share the leading extent K:

    node.send_output("rois", tensor.crops(frame, boxes, (128, 64), axes=(0, 1)))
    node.send_output("out", {"crop": tensor.crops(frame, boxes, (128, 64), axes=(0, 1)),
                             "box": boxes, "cls": cls})

`from_numpy_crops` is the statement of record.  Not offered: fractional boxes (ROI-align), rotated
boxes, a size per box, a batch index per box, int64 or float boxes, crops beside a `cast`,
`quantize`, `argmax` or `resize` in one dict, crops of or under `cast`, `quantize`, `argmax`,
`resize`, `ragged`, `take` or `masked`.
"""
from __future__ import annotations

from ctypes import c_int64

from ._lib import (REDUCE_ARGMAX, RESIZE_BILINEAR, RESIZE_NEAREST, Tensor, TensorAffine,
                   TensorCast, TensorField, TensorList, TensorMask, TensorQuant, TensorReduce,
                   TensorCrop, TensorResize, TensorTake)

_DL_CODES = {"i": 0, "u": 1, "f": 2, "b": 6, "c": 5}  # numpy dtype kind -> DLPack type code


def tensor_type(dtype, shape):
    """The pyarrow type of a tensor message of numpy `dtype` and `shape`."""
    import numpy as np
    import pyarrow as pa
    t = pa.from_numpy_dtype(np.dtype(dtype))
    for d in reversed(tuple(shape)[1:]):
        t = pa.list_(t, int(d))
    return t


def from_numpy(x):
    """The nested pyarrow array of a numpy array (copied to row-major order if it is a view)."""
    import numpy as np
    import pyarrow as pa
    x = np.asarray(x)
    if x.ndim < 1:
        raise ValueError("a tensor message has at least one dimension")
    arr = pa.array(np.ascontiguousarray(x).reshape(-1))
    for d in reversed(x.shape[1:]):
        arr = pa.FixedSizeListArray.from_arrays(arr, int(d))
    return arr


def struct_type(fields):
    """The pyarrow type of a struct-of-tensors message: `fields` maps each name to the
    `(dtype, shape)` of its tensor (the counterpart of `tensor_type`)."""
    import pyarrow as pa
    return pa.struct([pa.field(name, tensor_type(dtype, shape))
                      for name, (dtype, shape) in dict(fields).items()])


def from_numpy_struct(fields):
    """The pyarrow StructArray of a dict of numpy arrays that share their leading extent (the
    counterpart of `from_numpy`): what `send_output(output_id, fields)` puts on the wire."""
    import pyarrow as pa
    fields = dict(fields)
    if not fields:
        raise ValueError("a struct of tensors has at least one field")
    return pa.StructArray.from_arrays([from_numpy(v) for v in fields.values()], names=list(fields))


class Ragged:
    """A ragged batch: `values`, a tensor or a dict of tensors of leading extent N, and the
    partition of those N rows into B lists, as B + 1 `offsets` (what a received message carries,
    an int32 tensor of the values' library) or as B lengths (a batch built for sending may have
    either).  Build one for sending with `ragged`."""

    __slots__ = ("values", "offsets", "_lengths")

    def __init__(self, values, offsets=None, lengths=None):
        if (offsets is None) == (lengths is None):
            raise TypeError("a ragged batch takes exactly one of lengths and offsets")
        self.values, self.offsets, self._lengths = values, offsets, lengths

    def lengths(self):
        """The B list lengths, `offsets[1:] - offsets[:-1]` in the offsets' own library."""
        if self._lengths is not None:
            return self._lengths
        return self.offsets[1:] - self.offsets[:-1]

    def _bounds(self):
        part = self.offsets if self.offsets is not None else self._lengths
        part = part.tolist() if hasattr(part, "tolist") else list(part)
        if self.offsets is not None:
            return part
        out = [0]
        for n in part:
            out.append(out[-1] + n)
        return out

    def unbind(self):
        """The B lists as row views of `values` (dicts of views for a record).  The offsets are
        read on the host: on a device batch this synchronises with the stream that wrote them."""
        o = self._bounds()
        if isinstance(self.values, dict):
            return [{k: v[a:b] for k, v in self.values.items()} for a, b in zip(o, o[1:])]
        return [self.values[a:b] for a, b in zip(o, o[1:])]

    def __len__(self):
        part = self.offsets if self.offsets is not None else self._lengths
        return len(part) - (self.offsets is not None)

    def __repr__(self):
        return f"Ragged({len(self)} lists over {self.values!r})"


class Taken:
    """Rows taken along dimension 0: `values`, a tensor or a dict of tensors of leading extent N,
    and `index`, K row numbers into them.  It stands for `values[index]` in a send and copies
    nothing itself.  Build one with `take`."""

    __slots__ = ("values", "index")

    def __init__(self, values, index):
        self.values, self.index = values, index

    def __len__(self):
        return len(self.index)

    def __repr__(self):
        return f"Taken({len(self)} rows of {self.values!r})"


class Masked:
    """Rows selected along dimension 0: `values`, a tensor or a dict of tensors of leading extent
    N, and `mask`, N bool or uint8 elements.  It stands in a send for the N-row message whose
    first K rows are the selected ones and copies nothing itself.  Build one with `masked`."""

    __slots__ = ("values", "mask")

    def __init__(self, values, mask):
        self.values, self.mask = values, mask

    def __len__(self):
        return len(self.mask)

    def __repr__(self):
        return f"Masked({len(self)} rows of {self.values!r})"


def _has_cast(values):
    if isinstance(values, dict):
        return any(isinstance(v, Cast) for v in values.values())
    return isinstance(values, Cast)


def _has_quantized(values):
    if isinstance(values, dict):
        return any(isinstance(v, Quantized) for v in values.values())
    return isinstance(values, Quantized)


def _has_argmax(values):
    if isinstance(values, dict):
        return any(isinstance(v, Argmax) for v in values.values())
    return isinstance(values, Argmax)


def _has_crops(values):
    if isinstance(values, dict):
        return any(isinstance(v, Crops) for v in values.values())
    return isinstance(values, Crops)


def _has_resized(values):
    if isinstance(values, dict):
        return any(isinstance(v, Resized) for v in values.values())
    return isinstance(values, Resized)


def _cast_dtype(dtype):
    """(DLPack code, bits, name) of a cast or quantise destination given as a name, a numpy dtype
    or a torch dtype; the library refuses all but float16 and float32 (a cast) or uint8, int8,
    uint16 and int16 (a quantise)."""
    import numpy as np
    if str(dtype).startswith("torch."):
        name = str(dtype)[len("torch."):]
        if name == "bfloat16":
            return 4, 16, name
        dtype = {"half": "float16", "float": "float32", "double": "float64"}.get(name, name)
    try:
        dt = np.dtype(dtype)
    except TypeError:
        raise TypeError(f"cast: {dtype!r} is not a dtype") from None
    return _DL_CODES.get(dt.kind, 255), dt.itemsize * 8, dt.name


def _is_table(v):
    """Whether `v` (a scale or a bias) is a per-channel table and not one number."""
    if v is None or isinstance(v, (int, float)):
        return False
    if getattr(v, "ndim", None) == 0:
        return False
    return hasattr(v, "__len__") or hasattr(v, "__dlpack__")


class _Affine:
    """What `Cast` and `Quantized` share of the affine step `x * S + B`: `scale` and `bias` the
    scalars (None: absent or a table), `scale_table` and `bias_table` the per-channel tables as
    given (None: absent or a scalar), `axis` the dimension of `values` they run along, counted
    from the front (None: no table)."""

    __slots__ = ()

    def _set_affine(self, what, scale, bias, axis):
        import operator
        self.scale = self.bias = self.scale_table = self.bias_table = self.axis = None
        if axis is None:
            for name, v in (("scale", scale), ("bias", bias)):
                if _is_table(v) and not (name == "scale" and bias is None and what == "cast"):
                    # (a cast without bias and axis refuses a table as float() does, as before)
                    try:
                        v = float(v)
                    except (TypeError, ValueError):
                        raise TypeError(f"{what}: the {name} is one number; a per-channel {name} "
                                        "(a 1-D table) needs axis=") from None
                if v is not None:
                    setattr(self, name, float(v))
            return
        if not (_is_table(scale) or _is_table(bias)):
            raise TypeError(f"{what}: axis= goes with a per-channel scale or bias (a 1-D table); "
                            "with numbers alone leave it out")
        shape = getattr(self.values, "shape", None)
        if shape is None:
            raise TypeError(f"{what}: the values have no shape to count axis= in")
        axis = operator.index(axis)
        self.axis = axis + len(shape) if axis < 0 else axis  # (out of range: the send refuses it)
        for name, v in (("scale", scale), ("bias", bias)):
            if _is_table(v):
                setattr(self, name + "_table", v)
            elif v is not None:
                setattr(self, name, float(v))

    def _affine(self):
        """None, or the send's affine entry before its tables are described: (scale table or
        None, bias table or None, axis, scalar bias or None)."""
        if self.bias is None and self.scale_table is None and self.bias_table is None:
            return None
        return (self.scale_table, self.bias_table, self.axis or 0, self.bias)

    def _fill(self, a):
        a.dtype_code, a.dtype_bits = self._code, self._bits
        a.has_scale = 0 if self.scale is None else 1
        a.scale = 0.0 if self.scale is None else self.scale

    def _affine_repr(self):
        by = " * table" if self.scale_table is not None else \
            "" if self.scale is None else f" * {self.scale!r}"
        plus = " + table" if self.bias_table is not None else \
            "" if self.bias is None else f" + {self.bias!r}"
        return by + plus + ("" if self.axis is None else f" along axis {self.axis}")


class Cast(_Affine):
    """A tensor converted on send: `values`, a tensor, and the `dtype` it is sent as, after one
    optional multiplication by `scale` and one optional addition of `bias`, each a number or a
    per-channel table along `axis`.  It copies and converts nothing itself.  Build one with
    `cast`."""

    __slots__ = ("values", "dtype", "scale", "bias", "scale_table", "bias_table", "axis", "_code",
                 "_bits")
    _STRUCT = TensorCast

    def __init__(self, values, dtype, scale=None, bias=None, axis=None):
        self.values = values
        self._code, self._bits, self.dtype = _cast_dtype(dtype)
        self._set_affine("cast", scale, bias, axis)

    def _entry(self):
        return (self._code, self._bits, self.scale)

    def __repr__(self):
        return f"Cast({self.values!r}{self._affine_repr()} -> {self.dtype})"


def cast(values, dtype, scale=None, *, bias=None, axis=None):
    """`values` converted to `dtype` as a message: `values` a tensor of uint8, int8, uint16, int16,
    float16, bfloat16 or float32 (host memory or this node's HBM), `dtype` "float16" or "float32"
    (or the numpy or torch dtype), `scale` an optional finite factor applied in float32 first and
    `bias` an optional finite term added after it.  Either may be a 1-D table of one value per
    channel along `axis`, a dimension of `values` as given (negative: from the back), next to the
    values: a sequence, numpy array or CPU tensor with host values, a float32 tensor in this
    node's HBM with device values.  `send_output` sends it, on its own or as a value of a dict of
    tensors, as what `from_numpy_cast` states."""
    if isinstance(values, Quantized):
        raise TypeError("cast of a quantised tensor is not offered: a field is cast or quantised, "
                        "not both")
    if isinstance(values, Argmax):
        raise TypeError("cast of an argmax is not offered: give argmax the index dtype to send")
    if isinstance(values, Resized):
        raise TypeError("cast of a resize is not offered: give resize the dtype to send")
    if isinstance(values, Crops):
        raise TypeError("cast of crops is not offered: give crops the dtype to send")
    if isinstance(values, (Cast, Taken, Masked, Ragged, dict)):
        raise TypeError("cast converts one tensor: give a dict's fields a cast each; a cast under "
                        "ragged or take is not offered")
    return Cast(values, dtype, scale, bias, axis)


def _numpy_affine(y, scale, bias, axis):
    """`y * s32 + b32` in float32, the product rounded and then the sum: `scale` and `bias` None,
    a number or a 1-D table reshaped to broadcast along `axis` of `y`."""
    import numpy as np

    def term(v, name):
        if v is None:
            return None
        a = np.asarray(v, dtype=np.float32)
        if a.ndim == 0:
            return np.float32(a)
        if axis is None:
            raise TypeError(f"a per-channel {name} (a 1-D table) needs axis=")
        if a.ndim != 1 or len(a) != y.shape[axis]:
            raise ValueError(f"the {name} table has shape {a.shape}, the values have "
                             f"{y.shape[axis]} along axis {axis}")
        shape = [1] * y.ndim
        shape[axis] = len(a)
        return a.reshape(shape)
    s, b = term(scale, "scale"), term(bias, "bias")
    if s is not None:
        y = y * s
    if b is not None:
        y = y + b
    return y


def from_numpy_cast(x, dtype, scale=None, *, bfloat16=False, bias=None, axis=None):
    """The nested pyarrow array of `(x.astype(float32) * s32 + b32).astype(dtype)`, the statement
    of record of `cast` and the counterpart of `from_numpy`: what
    `send_output(output_id, cast(x, dtype, scale, bias=bias, axis=axis))` puts on the wire.  `s32`
    and `b32` are `scale` and `bias` as float32, a 1-D table reshaped to broadcast along `axis`;
    the product is rounded to float32, then the sum; an absent term is not applied.  `bfloat16`:
    `x` holds the bits of bfloat16 values as uint16 (numpy has no such dtype)."""
    import numpy as np
    x = np.asarray(x)
    if bfloat16:
        x = (x.astype(np.uint32) << 16).view(np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        y = _numpy_affine(x.astype(np.float32), scale, bias, axis)
        return from_numpy(y.astype(np.dtype(_cast_dtype(dtype)[2])))


class Quantized(_Affine):
    """A tensor quantised on send: `values`, a tensor, the integer `dtype` it is sent as, the
    optional `scale` it is multiplied by first, the optional `bias` added to the product (each a
    number or a per-channel table along `axis`) and the `zero_point` added last.  It copies and
    converts nothing itself.  Build one with `quantize`."""

    __slots__ = ("values", "dtype", "scale", "bias", "scale_table", "bias_table", "axis",
                 "zero_point", "_code", "_bits")
    _STRUCT = TensorQuant

    def __init__(self, values, dtype, scale=None, zero_point=0, bias=None, axis=None):
        import operator
        self.values = values
        self._code, self._bits, self.dtype = _cast_dtype(dtype)
        self._set_affine("quantize", scale, bias, axis)
        try:
            self.zero_point = operator.index(zero_point)
        except TypeError:
            raise TypeError(f"quantize: the zero point {zero_point!r} is not an integer (per-channel "
                            "zero points are not offered)") from None
        if not -2 ** 31 <= self.zero_point < 2 ** 31:
            raise ValueError(f"quantize: the zero point {self.zero_point} is outside every "
                             "destination's range")

    def _entry(self):
        return (self._code, self._bits, self.scale, self.zero_point)

    def _fill(self, a):
        super()._fill(a)
        a.zero_point = self.zero_point

    def __repr__(self):
        zp = "" if not self.zero_point else f" + {self.zero_point}"
        return f"Quantized({self.values!r}{self._affine_repr()}{zp} -> {self.dtype})"


def quantize(values, dtype, scale=None, zero_point=0, *, bias=None, axis=None):
    """`values` quantised to `dtype` as a message: `values` a tensor of uint8, int8, uint16, int16,
    float16, bfloat16 or float32 (host memory or this node's HBM), `dtype` "uint8", "int8",
    "uint16" or "int16" (or the numpy or torch dtype), `scale` an optional finite factor applied in
    float32 first, `bias` an optional finite term added after it — either may be a 1-D table of one
    value per channel along `axis`, as in `cast` — and `zero_point` one integer in the range of
    `dtype`.  `send_output` sends it, on its own or as a value of a dict of tensors, as what
    `from_numpy_quantize` states."""
    if isinstance(values, Argmax):
        raise TypeError("quantize of an argmax is not offered: give argmax the index dtype to "
                        "send")
    if isinstance(values, Resized):
        raise TypeError("quantize of a resize is not offered: give resize the dtype to send")
    if isinstance(values, Crops):
        raise TypeError("quantize of crops is not offered: give crops the dtype to send")
    if isinstance(values, (Quantized, Cast, Taken, Masked, Ragged, dict)):
        raise TypeError("quantize converts one tensor: give a dict's fields a quantize each; a "
                        "quantise of a cast, or under ragged, take or masked, is not offered")
    return Quantized(values, dtype, scale, zero_point, bias, axis)


def from_numpy_quantize(x, dtype, scale=None, zero_point=0, *, bfloat16=False, bias=None,
                        axis=None):
    """The nested pyarrow array of `x` quantised to `dtype`, the statement of record of `quantize`:
    what `send_output(output_id, quantize(x, dtype, scale, zero_point, bias=bias, axis=axis))`
    puts on the wire, `y = x.astype(float32) * s32 + b32` as in `from_numpy_cast`.  `bfloat16`:
    `x` holds the bits of bfloat16 values as uint16."""
    import numpy as np
    x = np.asarray(x)
    if bfloat16:
        x = (x.astype(np.uint32) << 16).view(np.float32)
    dt = np.dtype(_cast_dtype(dtype)[2])
    info = np.iinfo(dt)
    zp = int(zero_point)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        y = _numpy_affine(x.astype(np.float32), scale, bias, axis)
        r = np.rint(y)
        r = np.where(np.isnan(y), np.float32(0), r)
        r = np.clip(r, np.float32(info.min - zp), np.float32(info.max - zp))
        return from_numpy((r.astype(np.int32) + np.int32(zp)).astype(dt))


class Argmax:
    """A tensor reduced on send: `values`, a tensor, the `axis` whose maximum's index is sent
    (counted from the front) and the index `dtype`.  It reads and reduces nothing itself.  Build
    one with `argmax`."""

    __slots__ = ("values", "axis", "dtype", "_code", "_bits")
    _STRUCT = TensorReduce

    def __init__(self, values, axis, dtype="int64"):
        import operator
        self.values = values
        self._code, self._bits, self.dtype = _cast_dtype(dtype)
        axis = operator.index(axis)
        shape = getattr(values, "shape", None)
        if shape is None:
            raise TypeError("argmax: the values have no shape to count axis in")
        self.axis = axis + len(shape) if axis < 0 else axis  # (out of range: the send refuses it)
        if not -2 ** 31 <= self.axis < 2 ** 31:
            raise ValueError(f"argmax: axis {axis}")

    def _entry(self):
        return (REDUCE_ARGMAX, self.axis, self._code, self._bits)

    def _fill(self, a):
        a.op, a.axis, a.dtype_code, a.dtype_bits = self._entry()

    def __repr__(self):
        return f"Argmax({self.values!r} along axis {self.axis} -> {self.dtype})"


def argmax(values, axis, dtype="int64"):
    """The index of the maximum of `values` along `axis` as a message: `values` a tensor of uint8,
    int8, uint16, int16, float16, bfloat16 or float32 with at least two dimensions (host memory or
    this node's HBM, any strided view), `axis` one of its dimensions as given (negative: from the
    back), `dtype` "uint8", "uint16", "int32" or "int64" (or the numpy or torch dtype).
    `send_output` sends it, on its own or as a value of a dict of tensors, as what
    `from_numpy_argmax` states."""
    if isinstance(values, Resized):
        raise TypeError("argmax of a resize is not offered: reduce the resized tensor yourself, or "
                        "send the two in messages of their own")
    if isinstance(values, Crops):
        raise TypeError("argmax of crops is not offered: reduce the crops yourself, or send the "
                        "two in messages of their own")
    if isinstance(values, (Argmax, Cast, Quantized, Taken, Masked, Ragged, dict)):
        raise TypeError("argmax reduces one tensor: give a dict's fields an argmax each; an argmax "
                        "of a cast, a quantise, a take, a mask or a ragged batch is not offered")
    return Argmax(values, axis, dtype)


def from_numpy_argmax(x, axis, dtype="int64", *, bfloat16=False):
    """The nested pyarrow array of `np.argmax(x32, axis).astype(dtype)`, the statement of record
    of `argmax`: what `send_output(output_id, argmax(x, axis, dtype))` puts on the wire.  `x32` is
    `x` widened to float32, exact for every source; the first NaN wins, else the first maximum.
    `bfloat16`: `x` holds the bits of bfloat16 values as uint16 (numpy has no such dtype)."""
    import numpy as np
    x = np.asarray(x)
    if bfloat16:
        x = (x.astype(np.uint32) << 16).view(np.float32)
    if x.ndim < 2:
        raise ValueError("an argmax message reduces a tensor of at least two dimensions")
    dt = np.dtype(_cast_dtype(dtype)[2])
    if x.shape[axis] - 1 > np.iinfo(dt).max:
        raise ValueError(f"the index {x.shape[axis] - 1} does not fit {dt.name}")
    return from_numpy(np.argmax(x.astype(np.float32), axis).astype(dt))


_RESIZE_MODES = {"nearest": RESIZE_NEAREST, "bilinear": RESIZE_BILINEAR}


def letterbox(in_extents, size, anchor="center"):
    """`(inner, lead)` of the aspect-preserving fit of a source of extents `in_extents`
    `(Ia, Ib)` into an output of extents `size` `(Oa, Ob)`, in integer arithmetic only: the
    resized image has extents `inner = (Ra, Rb)` and starts at `lead = (pa, pb)` inside the
    output.  If `Oa * Ib <= Ob * Ia` the first axis is filled, `Ra = Oa` and
    `Rb = min(max((2 * Ib * Oa + Ia) // (2 * Ia), 1), Ob)` (the quotient rounded half up); else
    `Rb = Ob` and `Ra = min(max((2 * Ia * Ob + Ib) // (2 * Ib), 1), Oa)`.  `lead` is
    `((Oa - Ra) // 2, (Ob - Rb) // 2)` for `anchor="center"` and `(0, 0)` for `"start"`.
    (1080, 1920) into (640, 640) gives inner (360, 640), lead (140, 0).

    `resize(.., fit="letterbox")` places the image by this function, and a receiver uses the same
    function with the same arguments to map boxes found in the output back into the source:
    output coordinate `o` along an axis is source coordinate `(o - lead) * I / R`."""
    import operator
    try:
        (ia, ib), (oa, ob) = (tuple(operator.index(v) for v in p) for p in (in_extents, size))
    except (TypeError, ValueError):
        raise TypeError("letterbox: in_extents and size are two integers each") from None
    if min(ia, ib, oa, ob) < 1:
        raise ValueError(f"letterbox: extents {(ia, ib)} into {(oa, ob)}: every extent is at "
                         "least 1")
    if anchor not in ("center", "start"):
        raise ValueError(f"letterbox: anchor {anchor!r} is not offered: 'center' and 'start' are")
    if oa * ib <= ob * ia:
        ra, rb = oa, min(max((2 * ib * oa + ia) // (2 * ia), 1), ob)
    else:
        ra, rb = min(max((2 * ia * ob + ib) // (2 * ib), 1), oa), ob
    lead = ((oa - ra) // 2, (ob - rb) // 2) if anchor == "center" else (0, 0)
    return (ra, rb), lead


class _Prep(_Affine):
    """What `Resized` and `Crops` share of a model input's step: `_Affine`'s members — the terms
    of `r * S + B` before the conversion — and, for a resize, the placement: `inner` and `lead`
    (None: the image fills the output) and `fill`."""

    __slots__ = ()

    def _prep(self):
        """None (nothing is added), or the send's prep entry before its tables are described:
        (scale table or None, bias table or None, axis, scalar scale or None, scalar bias or
        None, inner0, inner1, lead0, lead1, fill)."""
        inner = getattr(self, "inner", None)
        if self.scale is None and self.bias is None and self.scale_table is None and \
                self.bias_table is None and inner is None:
            return None
        lead = (0, 0) if inner is None else self.lead
        return (self.scale_table, self.bias_table, self.axis or 0, self.scale, self.bias, *(inner or (0, 0)), *lead,
                float(getattr(self, "fill", 0.0)))

    def _prep_repr(self):
        inner = getattr(self, "inner", None)
        at = "" if inner is None else f", {inner} at {self.lead} in {self.fill!r}"
        return at + self._affine_repr()


class Resized(_Prep):
    """A tensor resized on send: `values`, a tensor, the two `axes` resized (counted from the
    front), their new extents `size`, the `mode` and the destination `dtype` (None: the source's
    own); for a model input also the terms of the affine step (`_Affine`'s members) and the
    placement `inner`, `lead` (None: the image fills the output) and `fill`.  It reads and resizes
    nothing itself.  Build one with `resize`."""

    __slots__ = ("values", "size", "axes", "mode", "dtype", "_mode", "_code", "_bits", "scale",
                 "bias", "scale_table", "bias_table", "axis", "inner", "lead", "fill")
    _STRUCT = TensorResize

    def __init__(self, values, size, axes=(-2, -1), mode="nearest", dtype=None, scale=None,
                 bias=None, axis=None, inner=None, lead=None, fill=0.0, what="resize"):
        import operator
        self.values = values
        shape = getattr(values, "shape", None)
        if shape is None:
            raise TypeError("resize: the values have no shape to count axes in")
        try:
            size = tuple(operator.index(v) for v in size)
            axes = tuple(operator.index(v) for v in axes)
        except TypeError:
            raise TypeError("resize: size and axes are two integers each") from None
        if len(size) != 2 or len(axes) != 2:
            raise TypeError("resize: size and axes are two integers each")
        if mode not in _RESIZE_MODES:
            raise ValueError(f"resize: mode {mode!r} is not offered: 'nearest' and 'bilinear' are")
        self.size = size
        # (out of range or equal: the send refuses them)
        self.axes = tuple(a + len(shape) if a < 0 else a for a in axes)
        if not all(-2 ** 31 <= a < 2 ** 31 for a in self.axes) or \
                not all(-2 ** 63 <= v < 2 ** 63 for v in size):
            raise ValueError(f"resize: axes {axes}, size {size}")
        self.mode, self._mode = mode, _RESIZE_MODES[mode]
        if dtype is None:
            self._code, self._bits, self.dtype = 0, 0, None
        else:
            self._code, self._bits, self.dtype = _cast_dtype(dtype)
        self._set_affine(what, scale, bias, axis)
        self.inner = self.lead = None
        try:
            self.fill = float(fill)
        except (TypeError, ValueError):
            raise TypeError(f"{what}: the fill is one number") from None
        if inner is not None:
            try:
                self.inner = tuple(operator.index(v) for v in inner)
                self.lead = tuple(operator.index(v) for v in ((0, 0) if lead is None else lead))
            except TypeError:
                raise TypeError(f"{what}: inner and lead are two integers each") from None
            if len(self.inner) != 2 or len(self.lead) != 2:
                raise TypeError(f"{what}: inner and lead are two integers each")
            # (out of range: the send refuses them)
            if not all(-2 ** 63 <= v < 2 ** 63 for v in self.inner + self.lead):
                raise ValueError(f"{what}: inner {self.inner}, lead {self.lead}")
        elif lead is not None:
            raise TypeError(f"{what}: lead= places an image of the extents inner=; give both")

    def _entry(self):
        return (self._mode, self.axes[0], self.axes[1], self.size[0], self.size[1], self._code,
                self._bits)

    def _fill(self, a):
        (a.mode, a.axis[0], a.axis[1], a.size[0], a.size[1], a.dtype_code,
         a.dtype_bits) = self._entry()

    def __repr__(self):
        return (f"Resized({self.values!r} axes {self.axes} -> {self.size}, {self.mode}"
                f"{self._prep_repr()}{'' if self.dtype is None else ' -> ' + self.dtype})")


def resize(values, size, *, axes=(-2, -1), mode="nearest", dtype=None, scale=None, bias=None,
           axis=None, fit="stretch", anchor="center", fill=0.0, inner=None, lead=None):
    """`values` with its two dimensions `axes` at the new extents `size` as a message: `values` a
    tensor of uint8, int8, uint16, int16, float16, bfloat16 or float32 with 2 to 8 dimensions (host
    memory or this node's HBM, any strided view), `axes` two of its dimensions as given (negative:
    from the back), `size` their new extents in that order, `mode` "nearest" or "bilinear"
    (half-pixel centres, no antialiasing), `dtype` "float16", "float32", "uint8", "int8", "uint16"
    or "int16" (or the numpy or torch dtype; None: the source's own).

    A model input in the same message: `scale` and `bias` are the terms of `r * S + B`, applied in
    float32 to the resized value before its conversion, each a finite number or a 1-D table of one
    value per channel along `axis` — a dimension of `values` as given that is not one of `axes` —
    living next to the values as `cast`'s tables do.  `fit="letterbox"` keeps the aspect: the
    image is resized to the `inner` extents that `letterbox(in_extents, size, anchor)` gives and
    placed at its `lead` inside an output of extents `size` whose other elements are `fill` (114
    for the usual grey), taken through the same `scale` and `bias`.  `inner=` and `lead=` give
    the placement directly (not together with `fit="letterbox"`).  `send_output` sends it, on its
    own or as a value of a dict of tensors, as what `from_numpy_resize` states."""
    if fit not in ("stretch", "letterbox"):
        raise ValueError(f"resize: fit {fit!r} is not offered: 'stretch' and 'letterbox' are")
    if fit == "letterbox":
        if inner is not None or lead is not None:
            raise TypeError("resize: fit='letterbox' computes inner and lead itself; give either "
                            "the fit or the placement")
        shape = getattr(values, "shape", None)
        if shape is None:
            raise TypeError("resize: the values have no shape to count axes in")
        try:
            src = tuple(shape[a] for a in axes)
        except (IndexError, TypeError):
            raise ValueError(f"resize: axes {tuple(axes)} of {len(shape)} dimensions") from None
        inner, lead = letterbox(src, size, anchor)
    if isinstance(values, Crops):
        raise TypeError("resize of crops is not offered: give crops the size to send")
    if isinstance(values, (Resized, Argmax, Cast, Quantized, Taken, Masked, Ragged, dict)):
        raise TypeError("resize resizes one tensor: give a dict's fields a resize each; a resize "
                        "of a cast, a quantise, an argmax, a take, a mask or a ragged batch is not "
                        "offered")
    return Resized(values, size, axes, mode, dtype, scale, bias, axis, inner, lead, fill)


def _resize_taps(n_in, n_out, mode):
    """(i0, i1, w0, w1) of every output coordinate of an axis of `n_in` source and `n_out` output
    steps: the statement's integer arithmetic and its two float32 divisions."""
    import numpy as np
    o = np.arange(n_out, dtype=np.int64)
    if mode == "nearest":
        i = (o * n_in) // n_out
        return i, i, None, None
    d = 2 * n_out
    n = np.maximum((2 * o + 1) * n_in - n_out, 0)
    q = n // d
    last = q >= n_in - 1
    i0 = np.where(last, n_in - 1, q)
    i1 = np.where(last, n_in - 1, q + 1)
    r = np.where(last, 0, n % d)
    w1 = r.astype(np.float32) / np.float32(d)
    w0 = (d - r).astype(np.float32) / np.float32(d)
    return i0, i1, w0, w1


def from_numpy_resize(x, size, *, axes=(-2, -1), mode="nearest", dtype=None, bfloat16=False,
                      scale=None, bias=None, axis=None, inner=None, lead=(0, 0), fill=0.0):
    """The nested pyarrow array of `x` resized, the statement of record of `resize`: what
    `send_output(output_id, resize(x, size, axes=axes, mode=mode, dtype=dtype))` puts on the wire.
    Every element is widened to float32; an axis of I source and O output steps reads at o the tap
    `(o * I) // O` (nearest) or blends the taps `q`, `q + 1` of `n = max((2 * o + 1) * I - O, 0)`,
    `q = n // (2 * O)` by `float32(n % (2 * O)) / float32(2 * O)` and its complement (bilinear; the
    last element alone where `q >= I - 1`), along the second of `axes` first, every product
    rounded to float32 and then every sum; the result goes to `dtype` as `from_numpy_cast` or
    `from_numpy_quantize` (no scale, zero point 0) takes it.  `bfloat16`: `x` holds the bits of
    bfloat16 values as uint16 (numpy has no such dtype) and `dtype` must be given.

    A model input (all absent by default).  Placement, `inner = (Ra, Rb)` with `1 <= R <= size`
    at `lead = (pa, pb)` with `0 <= p <= size - R`: the float32 value `r` of an output element at
    `(oa, ob)` along `axes` is the statement above with output extents `(Ra, Rb)` at
    `(oa - pa, ob - pb)` where `pa <= oa < pa + Ra` and `pb <= ob < pb + Rb`, and `float32(fill)`
    (finite) everywhere else.  Normalise, `scale`, `bias` and `axis` as `from_numpy_cast` takes
    them: `y = r * S[c] + B[c]` in float32, `c` the coordinate along `axis` (not one of `axes`),
    the product rounded and then the sum, an absent term not applied; padding goes through it like
    every other element.  Then the conversion of `y` as above, into the source's own integer dtype
    included."""
    return from_numpy(_numpy_resize(x, size, axes, mode, dtype, bfloat16, scale, bias, axis, inner,
                                    lead, fill))


def _numpy_resize(x, size, axes=(-2, -1), mode="nearest", dtype=None, bfloat16=False, scale=None,
                  bias=None, axis=None, inner=None, lead=(0, 0), fill=0.0):
    """`from_numpy_resize`'s values as a numpy array."""
    import numpy as np
    x = np.asarray(x)
    if bfloat16:
        if dtype is None:
            raise ValueError("a bfloat16 source names its destination dtype")
        x = (x.astype(np.uint32) << 16).view(np.float32)
    if mode not in _RESIZE_MODES:
        raise ValueError(f"mode {mode!r}")
    if not 2 <= x.ndim <= 8:
        raise ValueError("a resize message resizes a tensor of 2 to 8 dimensions")
    a, b = (ax + x.ndim if ax < 0 else ax for ax in axes)
    if a == b or not (0 <= a < x.ndim and 0 <= b < x.ndim):
        raise ValueError(f"axes {tuple(axes)} of {x.ndim} dimensions")
    for n in (x.shape[a], x.shape[b], size[0], size[1]):
        if not 1 <= n <= 32768:
            raise ValueError(f"extent {n}: 1 to 32768 are resized")
    dt = x.dtype if dtype is None else np.dtype(_cast_dtype(dtype)[2])
    if axis is not None:
        axis = axis + x.ndim if axis < 0 else axis
        if not 0 <= axis < x.ndim or axis in (a, b):
            raise ValueError(f"axis {axis}: a dimension of the values that is not resized")
    full = tuple(size)
    if inner is not None:
        if not np.isfinite(np.float32(fill)):
            raise ValueError(f"fill {fill!r} is not finite")
        for r, p, n in zip(inner, lead, size):
            if not (1 <= r <= n and 0 <= p <= n - r):
                raise ValueError(f"inner {tuple(inner)} at lead {tuple(lead)} does not lie inside "
                                 f"size {tuple(size)}")
        size = tuple(inner)
    v = x.astype(np.float32)
    a0, a1, wa0, wa1 = _resize_taps(x.shape[a], size[0], mode)
    b0, b1, wb0, wb1 = _resize_taps(x.shape[b], size[1], mode)

    def along(ax, w):  # a weight vector broadcast along axis `ax`
        shape = [1] * x.ndim
        shape[ax] = -1
        return w.reshape(shape)

    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if mode == "nearest":
            y = np.take(np.take(v, a0, axis=a), b0, axis=b)
        else:
            va0, va1 = np.take(v, a0, axis=a), np.take(v, a1, axis=a)
            wb0, wb1, wa0, wa1 = along(b, wb0), along(b, wb1), along(a, wa0), along(a, wa1)
            top = np.take(va0, b0, axis=b) * wb0 + np.take(va0, b1, axis=b) * wb1
            bot = np.take(va1, b0, axis=b) * wb0 + np.take(va1, b1, axis=b) * wb1
            y = top * wa0 + bot * wa1
        assert y.dtype == np.float32
        if inner is not None:
            shape = list(y.shape)
            shape[a], shape[b] = full
            placed = np.full(shape, np.float32(fill), np.float32)
            at = [slice(None)] * x.ndim
            at[a] = slice(lead[0], lead[0] + inner[0])
            at[b] = slice(lead[1], lead[1] + inner[1])
            placed[tuple(at)] = y
            y = placed
        y = _numpy_affine(y, scale, bias, axis)
        assert y.dtype == np.float32
        if dt.kind == "f":
            return y.astype(dt)
        info = np.iinfo(dt)
        r = np.where(np.isnan(y), np.float32(0), np.rint(y))
        r = np.clip(r, np.float32(info.min), np.float32(info.max))
        return r.astype(np.int32).astype(dt)


class Crops(_Prep):
    """Boxes cut from a frame and resized on send: `values`, the frame, `boxes`, the `[K, 4]`
    int32 tensor next to it, and what a `Resized` holds: the two `axes` cropped (counted from the
    front), the extents `size` of every crop, the `mode` and the destination `dtype` (None: the
    frame's own).  It reads, cuts and resizes nothing itself.  Build one with `crops`."""

    __slots__ = ("values", "boxes", "size", "axes", "mode", "dtype", "_resized", "scale", "bias",
                 "scale_table", "bias_table", "axis")
    _STRUCT = TensorCrop

    def __init__(self, values, boxes, size, axes=(-2, -1), mode="bilinear", dtype=None,
                 scale=None, bias=None, axis=None):
        try:
            r = Resized(values, size, axes, mode, dtype, scale, bias, axis, what="crops")
        except (TypeError, ValueError) as e:
            raise type(e)(str(e).replace("resize:", "crops:", 1)) from None
        for name in ("scale", "bias", "scale_table", "bias_table", "axis"):
            setattr(self, name, getattr(r, name))
        if not hasattr(boxes, "shape") and not isinstance(boxes, (list, tuple)):
            raise TypeError("crops: the boxes are a [K, 4] int32 tensor next to the frame")
        self._resized = r
        self.values, self.boxes = values, boxes
        self.size, self.axes, self.mode, self.dtype = r.size, r.axes, r.mode, r.dtype

    def _entry(self):
        """`Resized._entry()` and the boxes, which the node replaces by what it hands on."""
        return (*self._resized._entry(), self.boxes)

    def _fill(self, a, boxes=None):
        """Entry `a` (dora_tensor_crop); `boxes` a ctypes pointer to the boxes' `Tensor`, which
        the caller keeps alive."""
        self._resized._fill(a)
        if boxes is not None:
            a.boxes = boxes

    def __repr__(self):
        return (f"Crops({self.values!r} by {self.boxes!r} axes {self.axes} -> {self.size}, "
                f"{self.mode}{self._prep_repr()}"
                f"{'' if self.dtype is None else ' -> ' + self.dtype})")


def _no_crops_placement(kw):
    if kw:
        raise TypeError(f"crops: {', '.join(sorted(kw))}: placement for crops is not provided "
                        "(inner=, lead=, fit=, anchor= and fill= belong to resize: per-box aspect "
                        "would put a division per box on the device)"
                        if set(kw) <= {"inner", "lead", "fit", "anchor", "fill"} else
                        f"crops: unexpected keyword {sorted(kw)[0]!r}")


def crops(frame, boxes, size, *, axes=(-2, -1), mode="bilinear", dtype=None, scale=None,
          bias=None, axis=None, **placement):
    """The K `boxes` of `frame`, each cut out and brought to the extents `size`, as a message:
    `frame` a tensor of uint8, int8, uint16, int16, float16, bfloat16 or float32 with 2 to 7
    dimensions (host memory or this node's HBM, any strided view), `boxes` a dense `[K, 4]` int32
    tensor where the frame lives (never read on the host when that is HBM), row k
    `(a_lo, b_lo, a_hi, b_hi)`, half-open ranges along `axes[0]` and `axes[1]`; `size`, `axes`,
    `mode` and `dtype` as `resize` takes them.  Coordinates are clamped to the frame, a box that is
    then empty gives zeros.  `scale`, `bias` and `axis` normalise every crop as `resize` takes
    them, `axis` a dimension of `frame` as given (not counting K); an empty box stays zeros.
    Placement (`inner=`, `lead=`, `fit=`, `fill=`) is not provided for crops.  `send_output` sends
    it, on its own or as a value of a dict of tensors, as what `from_numpy_crops` states: a tensor
    of shape `(K,) + frame.shape` with the two extents replaced."""
    _no_crops_placement(placement)
    if isinstance(frame, (Crops, Resized, Argmax, Cast, Quantized, Taken, Masked, Ragged, dict)):
        raise TypeError("crops cuts boxes from one tensor: give a dict's fields their crops each; "
                        "crops of a cast, a quantise, an argmax, a resize, a take, a mask or a "
                        "ragged batch are not offered")
    return Crops(frame, boxes, size, axes, mode, dtype, scale, bias, axis)


def from_numpy_crops(x, boxes, size, *, axes=(-2, -1), mode="bilinear", dtype=None,
                     bfloat16=False, scale=None, bias=None, axis=None, **placement):
    """The nested pyarrow array of the crops of `x`, the statement of record of `crops`: what
    `send_output(output_id, crops(x, boxes, size, axes=axes, mode=mode, dtype=dtype))` puts on the
    wire.  With Ia, Ib the extents of `x` along `axes`, row k of `boxes` is clamped word by word,
    `a0 = min(max(a_lo, 0), Ia)`, `a1 = min(max(a_hi, 0), Ia)`, the same for b; crop k is all
    zeros where `a1 <= a0` or `b1 <= b0`, and else `from_numpy_resize` of
    `x[.., a0:a1, .., b0:b1, ..]`.  `bfloat16` as `from_numpy_resize` takes it.  `scale`, `bias`
    and `axis` (a dimension of `x`, not counting K) normalise every non-empty crop as
    `from_numpy_resize` states; every byte of an empty box's crop is zero whatever they are.
    Placement is not provided for crops."""
    _no_crops_placement(placement)
    return from_numpy(_numpy_crops(x, boxes, size, axes, mode, dtype, bfloat16, scale, bias, axis))


def _numpy_crops(x, boxes, size, axes=(-2, -1), mode="bilinear", dtype=None, bfloat16=False,
                 scale=None, bias=None, axis=None, **placement):
    """`from_numpy_crops`' values as a numpy array."""
    import numpy as np
    x = np.asarray(x)
    boxes = np.asarray(boxes)
    if boxes.size == 0:  # (an empty list is an array of float64)
        boxes = boxes.reshape(0, 4).astype(np.int32)
    if boxes.ndim != 2 or boxes.shape[1] != 4 or boxes.dtype.kind not in "iu":
        raise ValueError("boxes are [K, 4] integers")
    if not 2 <= x.ndim <= 7:
        raise ValueError("a crops message cuts a frame of 2 to 7 dimensions")
    a, b = (ax + x.ndim if ax < 0 else ax for ax in axes)
    if a == b or not (0 <= a < x.ndim and 0 <= b < x.ndim):
        raise ValueError(f"axes {tuple(axes)} of {x.ndim} dimensions")
    _no_crops_placement(placement)
    norm = dict(scale=scale, bias=bias, axis=axis)
    # (the refusals, shape and dtype)
    whole = _numpy_resize(x, size, axes, mode, dtype, bfloat16, **norm)
    out = np.zeros((boxes.shape[0],) + whole.shape, whole.dtype)
    ia, ib = x.shape[a], x.shape[b]
    for k, (alo, blo, ahi, bhi) in enumerate(boxes.tolist()):
        a0, a1 = min(max(alo, 0), ia), min(max(ahi, 0), ia)
        b0, b1 = min(max(blo, 0), ib), min(max(bhi, 0), ib)
        if a1 <= a0 or b1 <= b0:
            continue
        cut = [slice(None)] * x.ndim
        cut[a], cut[b] = slice(a0, a1), slice(b0, b1)
        out[k] = _numpy_resize(x[tuple(cut)], size, axes, mode, dtype, bfloat16, **norm)
    return out


def take(values, index):
    """`values[index]` along dimension 0 as a message: `values` a tensor or a dict of at most 8
    tensors sharing their leading extent N, `index` a 1-D sequence or tensor of K int32 or int64
    row numbers, 0 <= i < N, next to the values (host with host, this node's HBM with device
    tensors).  `send_output` sends it, bare or under `ragged`, as what `values[index]` would be."""
    if isinstance(values, (Taken, Masked, Ragged)):
        raise TypeError("take selects rows of a tensor or of a dict of tensors")
    if _has_cast(values):
        raise TypeError("cast under take is not offered: convert the taken rows with .to(dtype), "
                        "or send the cast without the take")
    if _has_quantized(values):
        raise TypeError("quantize under take is not offered: quantise the taken rows yourself, or "
                        "send the quantised tensor without the take")
    if _has_argmax(values):
        raise TypeError("argmax under take is not offered: reduce the taken rows yourself, or "
                        "send the argmax without the take")
    if _has_crops(values):
        raise TypeError("crops under take are not offered: crop the taken rows yourself, or send "
                        "the crops without the take")
    if _has_resized(values):
        raise TypeError("resize under take is not offered: resize the taken rows yourself, or "
                        "send the resize without the take")
    return Taken(values, index)


def masked(values, mask):
    """The rows of `values` that `mask` selects as a message: `values` a tensor or a dict of at
    most 8 tensors sharing their leading extent N, `mask` a 1-D dense sequence or tensor of N bool
    or uint8 elements next to the values (host with host, this node's HBM with device tensors),
    any non-zero element selecting its row.  `send_output` sends it, bare or under `ragged`, as
    what `from_numpy_masked` states: N rows, the K selected ones in front."""
    if isinstance(values, (Taken, Masked, Ragged)):
        raise TypeError("masked selects rows of a tensor or of a dict of tensors")
    if _has_cast(values):
        raise TypeError("cast under a mask is not offered: convert the values with .to(dtype), or "
                        "send the cast without the mask")
    if _has_quantized(values):
        raise TypeError("quantize under a mask is not offered: quantise the values yourself, or "
                        "send the quantised tensor without the mask")
    if _has_argmax(values):
        raise TypeError("argmax under a mask is not offered: reduce the values yourself, or send "
                        "the argmax without the mask")
    if _has_crops(values):
        raise TypeError("crops under a mask are not offered: crop the values yourself, or send "
                        "the crops without the mask")
    if _has_resized(values):
        raise TypeError("resize under a mask is not offered: resize the values yourself, or send "
                        "the resize without the mask")
    return Masked(values, mask)


def ragged(values, *, lengths=None, offsets=None):
    """The ragged batch of `values` (a tensor, or a dict of at most 8 tensors sharing their
    leading extent N, or rows of either taken by `take`: N is then the K taken rows; or rows of
    either selected by `masked`: the partition then describes the N source rows) cut into
    lists by exactly one of `lengths` (B of them) and `offsets` (B + 1): what `send_output` sends
    as one `List` message."""
    if _has_cast(values):
        raise TypeError("cast under ragged is not offered: convert the values with .to(dtype), or "
                        "send the cast without the partition")
    if _has_quantized(values):
        raise TypeError("quantize under ragged is not offered: quantise the values yourself, or "
                        "send the quantised tensor without the partition")
    if _has_argmax(values):
        raise TypeError("argmax under ragged is not offered: reduce the values yourself, or send "
                        "the argmax without the partition")
    if _has_crops(values):
        raise TypeError("crops under ragged are not offered: crop the values yourself, or send "
                        "the crops without the partition")
    if _has_resized(values):
        raise TypeError("resize under ragged is not offered: resize the values yourself, or send "
                        "the resize without the partition")
    return Ragged(values, offsets=offsets, lengths=lengths)


def ragged_type(values):
    """The pyarrow type of a ragged-batch message: `values` is the `(dtype, shape)` of a tensor
    or maps each field name to one (the counterpart of `struct_type`)."""
    import pyarrow as pa
    if isinstance(values, dict):
        return pa.list_(struct_type(values))
    dtype, shape = values
    return pa.list_(tensor_type(dtype, shape))


def _host_offsets(n, lengths, offsets):
    import numpy as np
    if (offsets is None) == (lengths is None):
        raise TypeError("a ragged batch takes exactly one of lengths and offsets")
    if offsets is not None:
        o = np.asarray(offsets, dtype=np.int64).reshape(-1)
    else:
        o = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64).reshape(-1))])
    if len(o) < 1 or o[0] != 0 or o[-1] != n or (np.diff(o) < 0).any():
        raise ValueError(f"the partition does not cut {n} rows into lists")
    return o.astype(np.int32)


def from_numpy_ragged(values, *, lengths=None, offsets=None):
    """The pyarrow ListArray of a numpy array, or of a dict of numpy arrays sharing their leading
    extent, cut by `lengths` or `offsets` (the counterpart of `from_numpy_struct`): what
    `send_output(output_id, ragged(values, ..))` puts on the wire."""
    import pyarrow as pa
    child = from_numpy_struct(values) if isinstance(values, dict) else from_numpy(values)
    o = _host_offsets(len(child), lengths, offsets)
    return pa.ListArray.from_arrays(pa.array(o, pa.int32()), child)


def from_numpy_take(values, index, *, lengths=None, offsets=None):
    """The pyarrow array of rows `index` of a numpy array or of a dict of numpy arrays sharing
    their leading extent, cut into lists when `lengths` or `offsets` is given: `from_numpy`,
    `from_numpy_struct` or `from_numpy_ragged` of `values[index]`, what
    `send_output(output_id, take(values, index))` (under `ragged` with a partition) puts on the
    wire.  Row numbers outside [0, N) are refused; there is no negative wrap-around."""
    import numpy as np
    index = np.asarray(index).reshape(-1)
    if index.size == 0:
        index = index.astype(np.int64)
    if index.dtype.kind not in "iu":
        raise TypeError(f"the index holds {index.dtype}, not integers")
    record = isinstance(values, dict)
    cols = {k: np.asarray(v) for k, v in values.items()} if record else {"": np.asarray(values)}
    for name, v in cols.items():
        if v.ndim < 1:
            raise ValueError("a tensor message has at least one dimension")
        bad = np.flatnonzero((index < 0) | (index >= v.shape[0]))
        if len(bad):
            raise IndexError(f"index word {bad[0]} is {index[bad[0]]}, outside the {v.shape[0]} "
                             "rows of the values")
    taken = {k: v[index] for k, v in cols.items()}
    taken = taken if record else taken[""]
    if lengths is not None or offsets is not None:
        return from_numpy_ragged(taken, lengths=lengths, offsets=offsets)
    return from_numpy_struct(taken) if record else from_numpy(taken)


def from_numpy_masked(values, mask, *, lengths=None, offsets=None):
    """The pyarrow ListArray `send_output(output_id, masked(values, mask))` (under `ragged` with
    a partition) puts on the wire, wherever the values live: the child is `values` (a numpy array
    or a dict of numpy arrays sharing N) compacted by `mask` and zero-padded back to N rows, the
    offsets are `C[p]` — `p` the offsets of the partition of the N source rows (`[0, N]` without
    one), `C[i]` the number of selected rows among rows [0, i)."""
    import numpy as np
    import pyarrow as pa
    mask = np.asarray(mask)
    if mask.ndim != 1 or mask.dtype not in (np.bool_, np.uint8):
        raise TypeError(f"the mask is {mask.ndim}-D {mask.dtype}, not 1-D bool or uint8")
    keep = mask != 0
    record = isinstance(values, dict)
    cols = {k: np.asarray(v) for k, v in values.items()} if record else {"": np.asarray(values)}
    padded = {}
    for name, v in cols.items():
        if v.ndim < 1:
            raise ValueError("a tensor message has at least one dimension")
        if v.shape[0] != len(keep):
            raise ValueError(f"the mask has {len(keep)} elements, the values have {v.shape[0]} rows")
        out = np.zeros(v.shape, v.dtype)
        out[:int(keep.sum())] = v[keep]
        padded[name] = out
    child = from_numpy_struct(padded) if record else from_numpy(padded[""])
    n = len(keep)
    p = _host_offsets(n, lengths, offsets) if lengths is not None or offsets is not None \
        else np.array([0, n], np.int32)
    c = np.concatenate([[0], np.cumsum(keep)]).astype(np.int32)
    return pa.ListArray.from_arrays(pa.array(c[p], pa.int32()), child)


def to_numpy(arr):
    """The numpy array of a nested pyarrow array (a host receiver's `event["value"]`): shape
    `(len, s1, .., sk)`; of a struct of tensor columns, the dict `{name: array}`; of a List over
    either, the `Ragged` of the child's values and this array's int32 offsets, which index them.
    Nulls at any level, the struct's and the list's own included, are refused."""
    import pyarrow as pa
    if pa.types.is_list(arr.type):
        if arr.null_count:
            raise TypeError("a tensor message has no nulls")
        import numpy as np
        return Ragged(to_numpy(arr.values), offsets=np.array(arr.offsets, dtype=np.int32))
    if pa.types.is_struct(arr.type):
        if arr.null_count:
            raise TypeError("a tensor message has no nulls")
        # (field(i) of a sliced struct is the whole child: flatten() gives this slice's)
        return {arr.type.field(i).name: to_numpy(col) for i, col in enumerate(arr.flatten())}
    shape = [len(arr)]
    while pa.types.is_fixed_size_list(arr.type):
        if arr.null_count:
            raise TypeError("a tensor message has no nulls")
        shape.append(arr.type.list_size)
        arr = arr.flatten()  # the values of this array's own slice
    if arr.null_count:
        raise TypeError("a tensor message has no nulls")
    return arr.to_numpy(zero_copy_only=False).reshape(shape)


def to_torch(value):
    """The torch tensor of a received tensor message: zero-copy over the HBM sample for a device
    receiver's `event["value"]` (DLPack, kDLROCM; the tensor keeps the input alive), a copy of
    the nested pyarrow array for a host receiver's.  A struct of tensor columns gives the dict
    `{name: tensor}`, each a view of the one sample; a List over either gives `Ragged(values,
    offsets)`, on a device receiver both zero-copy over the one sample.  Nulls at any level are
    refused."""
    import torch
    import pyarrow as pa
    t = getattr(value, "type", None)
    if t is not None and pa.types.is_list(t):
        if hasattr(value, "list_values"):  # a DeviceArray: zero-copy child and offsets
            offsets = torch.from_dlpack(value.list_offsets())
            return Ragged(to_torch(value.list_values()), offsets=offsets)
        import numpy as np
        r = to_numpy(value)
        vals = r.values
        vals = ({k: torch.from_numpy(np.array(x)) for k, x in vals.items()}
                if isinstance(vals, dict) else torch.from_numpy(np.array(vals)))
        return Ragged(vals, offsets=torch.from_numpy(r.offsets))
    if t is not None and pa.types.is_struct(t):
        if hasattr(value, "field_views"):  # a DeviceArray: zero-copy children
            return {name: torch.from_dlpack(v) for name, v in value.field_views().items()}
        import numpy as np
        return {name: torch.from_numpy(np.array(x)) for name, x in to_numpy(value).items()}
    if hasattr(value, "__dlpack__"):
        return torch.from_dlpack(value)
    import numpy as np
    return torch.from_numpy(np.array(to_numpy(value)))


def _describe(ptr: int, shape, strides, dtype, byte_offset: int = 0) -> tuple:
    """A `dora_tensor` over `ptr` (strides in elements, or None for row-major) and the ctypes
    arrays it points at, which the caller keeps alive with it."""
    import numpy as np
    dt = np.dtype(dtype)
    t = Tensor()
    t.data = ptr
    t.byte_offset = byte_offset
    t.dtype_code = _DL_CODES.get(dt.kind, 255)
    t.dtype_bits = dt.itemsize * 8
    t.dtype_lanes = 1
    t.ndim = len(shape)
    sh = (c_int64 * max(len(shape), 1))(*shape)
    t.shape = sh
    st = None
    if strides is not None:
        st = (c_int64 * max(len(strides), 1))(*strides)
        t.strides = st
    return t, (sh, st)


def _describe_array(x) -> tuple:
    """`_describe` of an object with `__array_interface__` (a numpy array, read-only ones
    included, which numpy's own `__dlpack__` refuses to export)."""
    import numpy as np
    x = np.asarray(x)
    strides = [s // x.dtype.itemsize for s in x.strides]
    t, keep = _describe(x.__array_interface__["data"][0], x.shape, strides, x.dtype)
    return t, (x, keep)


def _describe_fields(names, tensors) -> tuple:
    """The `dora_tensor_field` array of `names` over the `Tensor`s of `_describe`, and what the
    caller keeps alive with it (besides each tensor's own keep)."""
    arr = (TensorField * len(names))()
    enc = [n.encode() for n in names]
    for k, (n, t) in enumerate(zip(enc, tensors)):
        arr[k].name = n
        arr[k].tensor = t
    return arr, (enc, tensors)


def _describe_entries(values, cls) -> "ctypes.Array":
    """The array of `cls._STRUCT` (dora_tensor_cast, _quant, _reduce or _resize) over `values`:
    entry k is filled by values[k] where that is a `cls` (`Cast`, `Quantized`, `Argmax`,
    `Resized`) and left zero — the field is sent as it is — where it is anything else."""
    arr = (cls._STRUCT * len(values))()
    for k, v in enumerate(values):
        if isinstance(v, cls):
            v._fill(arr[k])
    return arr


def _describe_affines(entries) -> tuple:
    """The `dora_tensor_affine` array of `entries`, each None (no affine step) or (scale table,
    bias table, axis, scalar bias) with a table a `Tensor` of `_describe` or None, and what the
    caller keeps alive with it."""
    from ctypes import pointer
    arr = (TensorAffine * len(entries))()
    keep = []
    for k, e in enumerate(entries):
        if e is None:
            continue
        s, b, axis, bias = e
        if s is not None:
            arr[k].scale = pointer(s)
        if b is not None:
            arr[k].bias = pointer(b)
        arr[k].axis = axis
        arr[k].has_bias = 0 if bias is None else 1
        arr[k].bias_value = 0.0 if bias is None else bias
        keep.append((s, b))
    return arr, keep


def _describe_list(names, tensors, partition, form, partition_device) -> tuple:
    """The `dora_tensor_list` over the `Tensor`s of `_describe` (`names` None: the one bare
    tensor) and the partition's `Tensor`, and what the caller keeps alive with it."""
    arr = (TensorField * len(tensors))()
    enc = [n.encode() for n in names] if names is not None else [None] * len(tensors)
    for k, (n, t) in enumerate(zip(enc, tensors)):
        arr[k].name = n
        arr[k].tensor = t
    lst = TensorList()
    lst.fields = arr
    lst.n = len(tensors)
    lst.partition = partition
    lst.partition_form = form
    lst.partition_device = partition_device
    return lst, (arr, enc, tensors, partition)


def _describe_take(names, tensors, index, index_device, partition, form,
                   partition_device) -> tuple:
    """The `dora_tensor_take` over the `Tensor`s of `_describe` (`names` None: the one bare
    tensor), the index's `Tensor` and the partition's (None: no lists), and what the caller keeps
    alive with it."""
    from ctypes import pointer
    arr = (TensorField * len(tensors))()
    enc = [n.encode() for n in names] if names is not None else [None] * len(tensors)
    for k, (n, t) in enumerate(zip(enc, tensors)):
        arr[k].name = n
        arr[k].tensor = t
    tk = TensorTake()
    tk.fields = arr
    tk.n = len(tensors)
    tk.index = index
    tk.index_device = index_device
    if partition is not None:
        tk.partition = pointer(partition)
    tk.partition_form = form
    tk.partition_device = partition_device
    return tk, (arr, enc, tensors, index, partition)


def _describe_mask(names, tensors, mask, mask_device, partition, form,
                   partition_device) -> tuple:
    """The `dora_tensor_mask` over the `Tensor`s of `_describe` (`names` None: the one bare
    tensor), the mask's `Tensor` and the partition's (None: one list), and what the caller keeps
    alive with it."""
    from ctypes import pointer
    arr = (TensorField * len(tensors))()
    enc = [n.encode() for n in names] if names is not None else [None] * len(tensors)
    for k, (n, t) in enumerate(zip(enc, tensors)):
        arr[k].name = n
        arr[k].tensor = t
    mk = TensorMask()
    mk.fields = arr
    mk.n = len(tensors)
    mk.mask = mask
    mk.mask_device = mask_device
    if partition is not None:
        mk.partition = pointer(partition)
    mk.partition_form = form
    mk.partition_device = partition_device
    return mk, (arr, enc, tensors, mask, partition)


__all__ = ["tensor_type", "struct_type", "ragged_type", "from_numpy", "from_numpy_struct",
           "from_numpy_ragged", "from_numpy_take", "from_numpy_masked", "to_numpy", "to_torch",
           "Ragged", "ragged", "Taken", "take", "Masked", "masked", "Cast", "cast",
           "from_numpy_cast", "Quantized", "quantize", "from_numpy_quantize", "Argmax", "argmax",
           "from_numpy_argmax", "Resized", "resize", "from_numpy_resize", "Crops", "crops",
           "from_numpy_crops", "letterbox"]
