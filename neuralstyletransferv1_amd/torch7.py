"""Torch7 `.t7` fast-style networks (Johnson's Lua models: `*_eccv16.t7`, `instance_norm/*.t7`) on the engine.

The reference runs them one frame at a time through OpenCV DNN on the CPU (`cv2.dnn.readNetFromTorch`,
pipeline.py:445-478, 583-596).  Here the file is read on the host, matched against the one published
architecture, and run as the engine's NST_ARCH_TORCH7_IN / NST_ARCH_TORCH7_BN program:

  read_t7(path)        Torch7 binary serialisation -> Python objects (tables, tensors, `T7Object` modules)
  match_network(root)  the module tree -> ("in" | "bn", canonical parameter dict), or an NstError that names the
                       first thing that differs from the published architecture
  Torch7Net.from_t7    the nn.Module surface the pipeline's slots use

Parity with OpenCV is unpinned: neither cv2 nor a published .t7 file is available to the tests, which pin the
engine to an independent torch-CPU interpreter of the same file (tests/t7_ref.py) instead.
"""
from __future__ import annotations

import struct
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import NstError, check, lib
from .engine import Engine, StylizationNet

# ----------------------------------------------------------------------------- the file format
TYPE_NIL, TYPE_NUMBER, TYPE_STRING, TYPE_TABLE, TYPE_TORCH, TYPE_BOOLEAN = 0, 1, 2, 3, 4, 5
TYPE_FUNCTION, TYPE_RECUR_FUNCTION, LEGACY_TYPE_RECUR_FUNCTION = 6, 8, 7

_STORAGE_DTYPES = {"Float": np.dtype("<f4"), "Double": np.dtype("<f8"), "Long": np.dtype("<i8"), "Int": np.dtype("<i4"),
                   "Short": np.dtype("<i2"), "Byte": np.dtype("u1"), "Char": np.dtype("i1")}
_MAX_DEPTH = 128   # nesting of the published nets is under 10; a damaged file must not exhaust the interpreter stack
_MAX_NDIM = 16


class T7Object:
    """A torch class instance that is neither a tensor nor a storage (an nn module): class name + field table."""

    def __init__(self, torch_class: str, version: int):
        self.torch_class = torch_class
        self.version = version
        self.fields = None

    def get(self, name, default=None):
        return self.fields.get(name, default) if isinstance(self.fields, dict) else default

    def __repr__(self):
        return f"T7Object({self.torch_class})"


class T7Function:
    """A serialised Lua function (skipped: only its upvalues are kept)."""

    def __init__(self):
        self.upvalues = None


def _tensor_kind(cls: str) -> Optional[Tuple[str, str]]:
    """'torch.CudaLongTensor' -> ('Tensor', 'Long'); None for other classes.  Cuda names read as their host twins."""
    if not cls.startswith("torch."):
        return None
    name = cls[len("torch."):]
    for what in ("Tensor", "Storage"):
        if name.endswith(what):
            el = name[:-len(what)]
            if el.startswith("Cuda"):
                el = el[len("Cuda"):] or "Float"
            if el in _STORAGE_DTYPES:
                return what, el
    return None


class _Reader:
    def __init__(self, data: bytes):
        self.d = data
        self.pos = 0
        self.memo: Dict[int, object] = {}
        self.depth = 0

    def take(self, n: int) -> bytes:
        if n < 0 or n > len(self.d) - self.pos:
            raise NstError(f".t7 truncated: {n} bytes wanted at offset {self.pos}, {len(self.d) - self.pos} left")
        b = self.d[self.pos:self.pos + n]
        self.pos += n
        return b

    def int(self) -> int:
        return struct.unpack("<i", self.take(4))[0]

    def long(self) -> int:
        return struct.unpack("<q", self.take(8))[0]

    def string(self) -> str:
        n = self.int()
        if n < 0:
            raise NstError(f".t7 damaged: string length {n} at offset {self.pos - 4}")
        return self.take(n).decode("latin-1")

    def obj(self):
        self.depth += 1
        if self.depth > _MAX_DEPTH:
            raise NstError(f".t7 damaged: objects nested deeper than {_MAX_DEPTH}")
        try:
            return self._obj()
        finally:
            self.depth -= 1

    def _obj(self):
        at = self.pos
        tag = self.int()
        if tag == TYPE_NIL:
            return None
        if tag == TYPE_NUMBER:
            return struct.unpack("<d", self.take(8))[0]
        if tag == TYPE_STRING:
            return self.string()
        if tag == TYPE_BOOLEAN:
            return self.int() == 1
        if tag not in (TYPE_TABLE, TYPE_TORCH, TYPE_FUNCTION, TYPE_RECUR_FUNCTION, LEGACY_TYPE_RECUR_FUNCTION):
            raise NstError(f".t7 damaged: unknown type tag {tag} at offset {at}")
        index = self.int()
        if index in self.memo:
            return self.memo[index]
        if tag == TYPE_TABLE:
            t: dict = {}
            self.memo[index] = t
            size = self.int()
            if size < 0 or size > (len(self.d) - self.pos) // 8:  # an entry is at least two 4-byte tags
                raise NstError(f".t7 damaged: table of {size} entries at offset {self.pos - 4}")
            for _ in range(size):
                k = self.obj()
                v = self.obj()
                if isinstance(k, float) and k == int(k):
                    k = int(k)
                try:
                    t[k] = v
                except TypeError:
                    raise NstError(f".t7 damaged: unhashable table key {type(k).__name__}") from None
            return t
        if tag in (TYPE_FUNCTION, TYPE_RECUR_FUNCTION, LEGACY_TYPE_RECUR_FUNCTION):
            f = T7Function()
            self.memo[index] = f
            n = self.int()
            if n < 0:
                raise NstError(f".t7 damaged: function of {n} bytes at offset {self.pos - 4}")
            self.take(n)
            f.upvalues = self.obj()
            return f
        # torch object
        s = self.string()
        version = 0
        cls = s
        if s.startswith("V "):
            try:
                version = int(s[2:])
            except ValueError:
                raise NstError(f".t7 damaged: version string {s!r}") from None
            cls = self.string()
        kind = _tensor_kind(cls)
        if kind is None:
            o = T7Object(cls, version)
            self.memo[index] = o
            o.fields = self.obj()
            return o
        what, el = kind
        dt = _STORAGE_DTYPES[el]
        if what == "Storage":
            size = self.long()
            if size < 0 or size > (len(self.d) - self.pos) // dt.itemsize:
                raise NstError(f".t7 truncated: storage of {size} x {dt.itemsize} bytes at offset {self.pos - 8}")
            arr = np.frombuffer(self.take(size * dt.itemsize), dtype=dt).copy()
            st = torch.from_numpy(arr)
            self.memo[index] = st
            return st
        ndim = self.int()
        if ndim < 0 or ndim > _MAX_NDIM:
            raise NstError(f".t7 damaged: tensor of {ndim} dimensions at offset {self.pos - 4}")
        sizes = [self.long() for _ in range(ndim)]
        strides = [self.long() for _ in range(ndim)]
        offset = self.long()
        storage = self.obj()
        if storage is None or ndim == 0:
            ten = torch.empty((0,), dtype=torch.from_numpy(np.empty(0, dt)).dtype)
            self.memo[index] = ten
            return ten
        if not isinstance(storage, torch.Tensor) or storage.dim() != 1:
            raise NstError(f".t7 damaged: {cls} at offset {at} holds no storage")
        if any(s < 0 for s in sizes) or any(s < 0 for s in strides) or offset < 1:
            raise NstError(f".t7 damaged: {cls} sizes {sizes} strides {strides} offset {offset}")
        numel = int(np.prod(sizes, dtype=np.float64))
        last = (offset - 1) + sum((s - 1) * k for s, k in zip(sizes, strides)) if numel > 0 else 0
        if numel > 0 and last >= storage.numel():
            raise NstError(f".t7 damaged: {cls} of sizes {sizes} reaches element {last} of a storage of {storage.numel()}")
        ten = torch.as_strided(storage, sizes, strides, offset - 1) if numel > 0 else storage.new_empty(sizes)
        self.memo[index] = ten
        return ten


def read_t7_bytes(data: bytes):
    """One serialised object (the file's root).  Damaged or truncated input raises NstError; nothing past the
    buffer is ever read."""
    try:
        return _Reader(bytes(data)).obj()
    except NstError:
        raise
    except (struct.error, ValueError, OverflowError, RecursionError, MemoryError, RuntimeError) as e:
        raise NstError(f".t7 damaged: {type(e).__name__}: {e}") from None


def read_t7(path):
    try:
        with open(path, "rb") as f:
            data = f.read()
    except OSError as e:
        raise NstError(f"cannot read {path}: {e}") from None
    return read_t7_bytes(data)


# ----------------------------------------------------------------------------- the matcher
CAFFE_MEAN_BGR = (103.939, 116.779, 123.68)


def _cls(m) -> str:
    return m.torch_class if isinstance(m, T7Object) else type(m).__name__


def _children(m, where: str) -> List[object]:
    mods = m.get("modules")
    if not isinstance(mods, dict):
        raise NstError(f"{where}: {_cls(m)} has no modules table")
    out = []
    for i in range(1, len(mods) + 1):
        if i not in mods:
            raise NstError(f"{where}: modules table is not an array (no entry {i})")
        out.append(mods[i])
    return out


def _num(m, name, default=None):
    v = m.get(name, default)
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        return default
    return v


def _tensor(m, name, where, numel=None) -> torch.Tensor:
    t = m.get(name)
    if not isinstance(t, torch.Tensor) or t.numel() == 0:
        raise NstError(f"{where}: {_cls(m)} has no {name} tensor")
    if numel is not None and t.numel() != numel:
        raise NstError(f"{where}: {name} has {t.numel()} elements, expected {numel}")
    return t.to(torch.float32).contiguous()


def _expect(m, cls: str, where: str):
    if _cls(m) != cls:
        raise NstError(f"{where}: expected {cls}, found {_cls(m)}")


def _conv(m, where, full, cin, cout, k, stride, pad, out: Dict[str, torch.Tensor], name: str):
    _expect(m, "nn.SpatialFullConvolution" if full else "nn.SpatialConvolution", where)
    got = {"nInputPlane": _num(m, "nInputPlane"), "nOutputPlane": _num(m, "nOutputPlane"), "kW": _num(m, "kW"),
           "kH": _num(m, "kH"), "dW": _num(m, "dW", 1), "dH": _num(m, "dH", 1), "padW": _num(m, "padW", 0),
           "padH": _num(m, "padH", 0)}
    want = {"nInputPlane": cin, "nOutputPlane": cout, "kW": k, "kH": k, "dW": stride, "dH": stride, "padW": pad, "padH": pad}
    if full:
        got.update(adjW=_num(m, "adjW", 0), adjH=_num(m, "adjH", 0))
        want.update(adjW=1, adjH=1)
    for key, w in want.items():
        if got[key] != w:
            raise NstError(f"{where}: {_cls(m)} {key} is {got[key]}, expected {w}")
    n = cin * cout * k * k
    wt = _tensor(m, "weight", where, n)
    # conv: [out, in, kh, kw] or legacy 2-D [out, in*kh*kw] (the same order); full conv: [in, out, kh, kw]
    out[name + ".weight"] = wt.reshape(cin, cout, k, k) if full else wt.reshape(cout, cin, k, k)
    out[name + ".bias"] = _tensor(m, "bias", where, cout).reshape(cout)


def _norm(m, where, c, kind: Optional[str], out: Dict[str, torch.Tensor], name: str) -> str:
    cls = _cls(m)
    this = {"nn.InstanceNormalization": "in", "nn.SpatialBatchNormalization": "bn"}.get(cls)
    if this is None:
        raise NstError(f"{where}: expected nn.InstanceNormalization or nn.SpatialBatchNormalization, found {cls}")
    if kind is not None and this != kind:
        raise NstError(f"{where}: mixed norm kinds: {cls} after "
                       f"{'nn.InstanceNormalization' if kind == 'in' else 'nn.SpatialBatchNormalization'} layers")
    eps = _num(m, "eps", 1e-5)
    if not eps >= 0:
        raise NstError(f"{where}: {cls} eps is {eps}")
    if this == "in":  # weight, bias, eps; an inner `bn` member (the implementation's helper module) is ignored
        out[name + ".weight"] = _tensor(m, "weight", where, c).reshape(c)
        out[name + ".bias"] = _tensor(m, "bias", where, c).reshape(c)
    else:
        affine = m.get("affine", True) is not False and isinstance(m.get("weight"), torch.Tensor)
        out[name + ".weight"] = _tensor(m, "weight", where, c).reshape(c) if affine else torch.ones(c)
        out[name + ".bias"] = _tensor(m, "bias", where, c).reshape(c) if affine else torch.zeros(c)
        out[name + ".running_mean"] = _tensor(m, "running_mean", where, c).reshape(c)
        if isinstance(m.get("running_var"), torch.Tensor) and m.get("running_var").numel() > 0:
            out[name + ".running_var"] = _tensor(m, "running_var", where, c).reshape(c)
        else:  # legacy files keep running_std = 1 / sqrt(var + eps)
            std = _tensor(m, "running_std", where, c).reshape(c).to(torch.float64)
            if not bool((std > 0).all()):
                raise NstError(f"{where}: running_std has a non-positive entry")
            out[name + ".running_var"] = (1.0 / (std * std) - float(eps)).to(torch.float32)
    out[name + ".eps"] = torch.tensor([float(eps)], dtype=torch.float32)
    return this


def match_network(root) -> Tuple[str, Dict[str, torch.Tensor]]:
    """The published fast-style architecture, exactly -> (norm kind, parameters under the engine's names:
    down1..3 / res1..5 / up1..2 / final as the NST_ARCH_NST layer table names them, `<norm>.eps`, for "bn" also
    `<norm>.running_mean` / `.running_var`, and `mul_constant`).  Anything else raises an NstError naming the first
    mismatch."""
    _expect(root, "nn.Sequential", "top level")
    mods = _children(root, "top level")
    P: Dict[str, torch.Tensor] = {}
    kind: Optional[str] = None
    pos = [0]

    def nxt(what: str):
        i = pos[0]
        if i >= len(mods):
            raise NstError(f"module {i + 1}: the network ends where {what} is expected")
        pos[0] += 1
        return mods[i], f"module {i + 1}"

    m, w = nxt("nn.SpatialReflectionPadding")
    _expect(m, "nn.SpatialReflectionPadding", w)
    for side in ("pad_l", "pad_r", "pad_t", "pad_b"):
        if _num(m, side) != 40:
            raise NstError(f"{w}: nn.SpatialReflectionPadding {side} is {_num(m, side)}, expected 40")

    def conv_norm_relu(name, full, cin, cout, k, stride, pad):
        nonlocal kind
        m, w = nxt(name + " conv")
        _conv(m, w, full, cin, cout, k, stride, pad, P, name + ".conv")
        m, w = nxt(name + " norm")
        kind = _norm(m, w, cout, kind, P, name + ".norm")
        m, w = nxt("nn.ReLU")
        _expect(m, "nn.ReLU", w)

    conv_norm_relu("down1", False, 3, 32, 9, 1, 4)
    conv_norm_relu("down2", False, 32, 64, 3, 2, 1)
    conv_norm_relu("down3", False, 64, 128, 3, 2, 1)
    for r in range(1, 6):
        blk, w = nxt(f"residual block {r}")
        _expect(blk, "nn.Sequential", w)
        parts = _children(blk, w)
        if len(parts) != 2:
            raise NstError(f"{w}: residual block of {len(parts)} modules, expected nn.ConcatTable + nn.CAddTable")
        _expect(parts[0], "nn.ConcatTable", w + ".1")
        _expect(parts[1], "nn.CAddTable", w + ".2")
        br = _children(parts[0], w + ".1")
        if len(br) != 2:
            raise NstError(f"{w}.1: nn.ConcatTable of {len(br)} branches, expected 2")
        _expect(br[0], "nn.Sequential", w + ".1.1")
        _expect(br[1], "nn.ShaveImage", w + ".1.2")
        if _num(br[1], "size") != 2:
            raise NstError(f"{w}.1.2: nn.ShaveImage size is {_num(br[1], 'size')}, expected 2")
        seq = _children(br[0], w + ".1.1")
        if len(seq) != 5:
            raise NstError(f"{w}.1.1: branch of {len(seq)} modules, expected conv, norm, nn.ReLU, conv, norm")
        bw = w + ".1.1"
        _conv(seq[0], f"{bw}.1", False, 128, 128, 3, 1, 0, P, f"res{r}.conv1")
        kind = _norm(seq[1], f"{bw}.2", 128, kind, P, f"res{r}.norm1")
        _expect(seq[2], "nn.ReLU", f"{bw}.3")
        _conv(seq[3], f"{bw}.4", False, 128, 128, 3, 1, 0, P, f"res{r}.conv2")
        kind = _norm(seq[4], f"{bw}.5", 128, kind, P, f"res{r}.norm2")
    conv_norm_relu("up1", True, 128, 64, 3, 2, 1)
    conv_norm_relu("up2", True, 64, 32, 3, 2, 1)
    m, w = nxt("the output conv")
    _conv(m, w, False, 32, 3, 9, 1, 4, P, "final")
    m, w = nxt("nn.Tanh")
    _expect(m, "nn.Tanh", w)
    m, w = nxt("nn.MulConstant")
    _expect(m, "nn.MulConstant", w)
    c = _num(m, "constant_scalar")
    if c is None:
        raise NstError(f"{w}: nn.MulConstant has no constant_scalar")
    P["mul_constant"] = torch.tensor([float(c)], dtype=torch.float32)
    if pos[0] < len(mods) and _cls(mods[pos[0]]) == "nn.TotalVariation":  # identity in the forward pass
        pos[0] += 1
    if pos[0] < len(mods):
        raise NstError(f"module {pos[0] + 1}: unexpected {_cls(mods[pos[0]])} after the network's tail")
    return kind, P


def load_t7(path) -> Tuple[str, Dict[str, torch.Tensor]]:
    return match_network(read_t7(path))


def output_side(h: int) -> int:
    """Output side length for an input side h: 4 * (h3 - 20) (= h when h % 4 == 0)."""
    h1 = h + 80
    h2 = (h1 - 1) // 2 + 1
    h3 = (h2 - 1) // 2 + 1
    return 4 * (h3 - 20)


# ----------------------------------------------------------------------------- the module surface
class Torch7Engine(Engine):
    """An Engine whose frames always go through NST_PRESET_TORCH7: the reference's _torch7_forward_openv ignores
    io_preset.  Toward the rest of the pipeline the slot is a raw_01 source: its float32 output is frame / 255
    (RGB planes), what to_tensor(pil_out).clamp(0, 1) hands on at pipeline.py:1443."""

    def forward_into(self, x, x_fmt, n, h, w, pid, y, y_fmt) -> None:
        if min(h, w) <= 40:
            raise NstError(f"Torch7 nets reflect-pad by 40 px: the frame's sides must exceed 40, got {h}x{w}")
        super().forward_into(x, x_fmt, n, h, w, 0 if pid == 0 else _lib.NST_PRESET_TORCH7, y, y_fmt)

    def stylize_u8(self, frames: torch.Tensor, preset: str = "caffe_bgr") -> torch.Tensor:
        _lib.require_gpu_tensor(frames, "frames")
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
            raise NstError(f"expected uint8 [N,H,W,3] frames, got {frames.dtype} {tuple(frames.shape)}")
        frames = frames.contiguous()
        n, h, w, _ = frames.shape
        if min(h, w) <= 40:
            raise NstError(f"Torch7 nets reflect-pad by 40 px: the frame's sides must exceed 40, got {h}x{w}")
        oh, ow = self.output_hw(h, w)
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=self.device)
        if (oh, ow) == (h, w):
            self.forward_into(frames, _lib.NST_IO_U8_NHWC, n, h, w, _lib.NST_PRESET_TORCH7, out, _lib.NST_IO_U8_NHWC)
            return out
        # the content-size fit of pipeline.py:1512-1516 over out01 = frame / 255
        y = torch.empty((n, 3, oh, ow), dtype=torch.float32, device=self.device)
        self.forward_into(frames, _lib.NST_IO_U8_NHWC, n, h, w, _lib.NST_PRESET_TORCH7, y, _lib.NST_IO_F32_NCHW)
        check(lib().nst_decode_resize_u8(y.data_ptr(), n, oh, ow, _lib.PRESETS["raw_01"], out.data_ptr(), h, w,
                                         _lib.stream_ptr(self.device)), "nst_decode_resize_u8")
        return out


class Torch7Net(StylizationNet):
    """A Torch7 fast-style network.  forward(X): the mean-subtracted BGR blob [N,3,H,W] -> tanh(.) * constant, what
    net.forward() returns in the reference (pipeline.py:466); stylize_frames: uint8 RGB frames -> uint8 RGB frames
    (the preset is ignored, as _torch7_forward_openv ignores it)."""

    ENGINE_CLS = Torch7Engine

    def __init__(self, kind: str, params: Dict[str, torch.Tensor]):
        super().__init__()
        if kind not in ("in", "bn"):
            raise NstError(f"norm kind must be 'in' or 'bn', got {kind!r}")
        self.norm_kind = kind
        self.ARCH = _lib.NST_ARCH_TORCH7_IN if kind == "in" else _lib.NST_ARCH_TORCH7_BN
        self._t7_params = {k: v.detach().to("cpu", torch.float32).contiguous() for k, v in params.items()}
        self.mul_constant = float(self._t7_params["mul_constant"][0])
        self.register_buffer("_device_anchor", torch.zeros(1), persistent=False)

    @classmethod
    def from_t7(cls, path) -> "Torch7Net":
        kind, params = load_t7(path)
        return cls(kind, params)

    def _engine_state(self) -> Dict[str, torch.Tensor]:
        return self._t7_params

    def _module_device(self) -> torch.device:
        return self._device_anchor.device

    def stylize_frames(self, frames_u8: torch.Tensor, io_preset: str = "caffe_bgr") -> torch.Tensor:
        return super().stylize_frames(frames_u8, io_preset)
