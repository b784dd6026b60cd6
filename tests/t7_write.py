"""A writer for Torch7 binary serialisation and the published fast-style architecture in its field variants
(test helper: neither a real .t7 file nor Torch7 itself is available to the tests).

Format (little-endian; int = int32, long = int64, number = float64): an int type tag, then
  0 nil | 1 number | 2 string (int length + bytes) | 5 boolean (int) | 3 table | 4 torch object
Tables and torch objects carry an int memo index first; an index written before stands for the same object.
"""
import struct

import numpy as np
import torch


class Obj:
    """A torch class instance: class name, field table, `versioned` header ("V 1" + name) or the legacy bare name."""

    def __init__(self, cls, fields, versioned=True):
        self.cls, self.fields, self.versioned = cls, fields, versioned


class Empty:
    """A tensor of no dimensions without a storage (a module's unset `output` / `gradInput`)."""


class _Writer:
    def __init__(self):
        self.out = bytearray()
        self.memo = {}

    def i(self, v):
        self.out += struct.pack("<i", v)

    def l(self, v):
        self.out += struct.pack("<q", v)

    def s(self, v):
        b = v.encode("latin-1")
        self.i(len(b))
        self.out += b

    def ref(self, tag, key):
        """tag + memo index; True if the object was written before (index only)."""
        self.i(tag)
        if key in self.memo:
            self.i(self.memo[key])
            return True
        self.memo[key] = len(self.memo) + 1
        self.i(self.memo[key])
        return False

    def header(self, cls, versioned):
        if versioned:
            self.s("V 1")
        self.s(cls)

    def obj(self, x, versioned=True):
        if x is None:
            self.i(0)
        elif isinstance(x, bool):
            self.i(5)
            self.i(1 if x else 0)
        elif isinstance(x, (int, float)):
            self.i(1)
            self.out += struct.pack("<d", float(x))
        elif isinstance(x, str):
            self.i(2)
            self.s(x)
        elif isinstance(x, (dict, list)):
            if self.ref(3, id(x)):
                return
            items = list(x.items()) if isinstance(x, dict) else [(k + 1, v) for k, v in enumerate(x)]
            self.i(len(items))
            for k, v in items:
                self.obj(k, versioned)
                self.obj(v, versioned)
        elif isinstance(x, Obj):
            if self.ref(4, id(x)):
                return
            self.header(x.cls, x.versioned)
            self.obj(x.fields, x.versioned)
        elif isinstance(x, Empty):
            if self.ref(4, id(x)):
                return
            self.header("torch.FloatTensor", versioned)
            self.i(0)
            self.l(1)
            self.i(0)  # nil storage
        elif isinstance(x, torch.Tensor):
            if self.ref(4, id(x)):
                return
            names = {torch.float32: ("Float", "<f4"), torch.float64: ("Double", "<f8"), torch.int64: ("Long", "<i8")}
            el, dt = names[x.dtype]
            self.header(f"torch.{el}Tensor", versioned)
            t = x.contiguous()
            self.i(t.dim())
            for v in t.shape:
                self.l(v)
            for v in t.stride():
                self.l(v)
            self.l(1)
            self.ref(4, ("storage", id(x)))
            self.header(f"torch.{el}Storage", versioned)
            self.l(t.numel())
            self.out += t.numpy().astype(dt).tobytes()
        else:
            raise TypeError(type(x))


def dumps(root) -> bytes:
    w = _Writer()
    w.obj(root)
    return bytes(w.out)


# ----------------------------------------------------------------------------- the architecture
def make_params(kind, seed=0, out_scale=1.0):
    """Canonical parameters from a fixed seed: He-scaled convs, gamma near 1, plausible running statistics, the
    output conv scaled by `out_scale`.  Keys as the engine names them (torch7.match_network)."""
    g = torch.Generator().manual_seed(1000 + seed)
    P = {}

    def conv(name, cin, cout, k, full=False, scale=1.0):
        std = (2.0 / (cin * k * k)) ** 0.5 * scale
        shape = (cin, cout, k, k) if full else (cout, cin, k, k)
        P[name + ".weight"] = torch.randn(shape, generator=g) * std
        P[name + ".bias"] = torch.randn(cout, generator=g) * 0.05

    def norm(name, c, var):
        P[name + ".weight"] = 1.0 + 0.1 * torch.randn(c, generator=g)
        P[name + ".bias"] = 0.1 * torch.randn(c, generator=g)
        P[name + ".eps"] = torch.tensor([1e-5])
        if kind == "bn":
            P[name + ".running_mean"] = 0.1 * var ** 0.5 * torch.randn(c, generator=g)
            P[name + ".running_var"] = var * (0.5 + torch.rand(c, generator=g))

    # the blob is BGR255 minus the Caffe mean: a variance of roughly 60^2 enters the first conv
    conv("down1.conv", 3, 32, 9)
    norm("down1.norm", 32, 2.0 * 60.0 ** 2)
    conv("down2.conv", 32, 64, 3)
    norm("down2.norm", 64, 1.0)
    conv("down3.conv", 64, 128, 3)
    norm("down3.norm", 128, 1.0)
    for r in range(1, 6):
        conv(f"res{r}.conv1", 128, 128, 3)
        norm(f"res{r}.norm1", 128, 1.0 + 0.5 * r)
        conv(f"res{r}.conv2", 128, 128, 3, scale=0.5)
        norm(f"res{r}.norm2", 128, 0.5)
    conv("up1.conv", 128, 64, 3, full=True)
    norm("up1.norm", 64, 1.0)
    conv("up2.conv", 64, 32, 3, full=True)
    norm("up2.norm", 32, 1.0)
    conv("final", 32, 3, 9, scale=out_scale)
    P["mul_constant"] = torch.tensor([150.0])
    return P


def build_tree(kind, P, *, running_std=False, weight2d=False, versioned=True, tv=False, affine=True, blocks=5):
    """The module tree of the published architecture around parameters P, in one of the field variants:
    BN with running_var or (legacy) running_std; InstanceNormalization with an inner `bn` whose weight and bias are
    the outer module's tensors (shared by memo index); 4-D or legacy 2-D conv weights; versioned or legacy class
    headers; with or without nn.TotalVariation."""
    def O(cls, fields):
        fields = dict(fields)
        fields.setdefault("train", False)
        fields.setdefault("output", Empty())
        return Obj(cls, fields, versioned)

    def conv(name, cin, cout, k, stride, pad, full=False):
        w = P[name + ".weight"]
        if weight2d and not full:
            w = w.reshape(cout, cin * k * k)
        f = {"nInputPlane": cin, "nOutputPlane": cout, "kW": k, "kH": k, "dW": stride, "dH": stride,
             "weight": w, "bias": P[name + ".bias"]}
        if pad or not weight2d:  # legacy files leave zero paddings out
            f.update(padW=pad, padH=pad)
        if full:
            f.update(adjW=1, adjH=1)
        return O("nn.SpatialFullConvolution" if full else "nn.SpatialConvolution", f)

    def norm(name):
        w, b, eps = P[name + ".weight"], P[name + ".bias"], float(P[name + ".eps"][0])
        if kind == "in":
            inner = O("nn.SpatialBatchNormalization", {"weight": w, "bias": b, "eps": eps, "affine": True,
                                                       "running_mean": torch.zeros(w.numel()),
                                                       "running_var": torch.ones(w.numel())})
            return O("nn.InstanceNormalization", {"weight": w, "bias": b, "eps": eps, "nOutput": w.numel(), "bn": inner})
        f = {"eps": eps, "affine": affine, "running_mean": P[name + ".running_mean"], "momentum": 0.1}
        if affine:
            f.update(weight=w, bias=b)
        if running_std:
            f["running_std"] = (P[name + ".running_var"].double() + eps).rsqrt().float()
        else:
            f["running_var"] = P[name + ".running_var"]
        return O("nn.SpatialBatchNormalization", f)

    def seq(mods):
        return O("nn.Sequential", {"modules": list(mods)})

    mods = [O("nn.SpatialReflectionPadding", {"pad_l": 40, "pad_r": 40, "pad_t": 40, "pad_b": 40}),
            conv("down1.conv", 3, 32, 9, 1, 4), norm("down1.norm"), O("nn.ReLU", {}),
            conv("down2.conv", 32, 64, 3, 2, 1), norm("down2.norm"), O("nn.ReLU", {}),
            conv("down3.conv", 64, 128, 3, 2, 1), norm("down3.norm"), O("nn.ReLU", {})]
    for r in range(1, blocks + 1):
        rr = min(r, 5)
        branch = seq([conv(f"res{rr}.conv1", 128, 128, 3, 1, 0), norm(f"res{rr}.norm1"), O("nn.ReLU", {}),
                      conv(f"res{rr}.conv2", 128, 128, 3, 1, 0), norm(f"res{rr}.norm2")])
        mods.append(seq([O("nn.ConcatTable", {"modules": [branch, O("nn.ShaveImage", {"size": 2})]}),
                         O("nn.CAddTable", {"inplace": False})]))
    mods += [conv("up1.conv", 128, 64, 3, 2, 1, full=True), norm("up1.norm"), O("nn.ReLU", {}),
             conv("up2.conv", 64, 32, 3, 2, 1, full=True), norm("up2.norm"), O("nn.ReLU", {}),
             conv("final", 32, 3, 9, 1, 4), O("nn.Tanh", {}),
             O("nn.MulConstant", {"constant_scalar": float(P["mul_constant"][0]), "inplace": False})]
    if tv:
        mods.append(O("nn.TotalVariation", {"strength": 1e-6}))
    return seq(mods)


VARIANTS = {
    "in": dict(kind="in"),
    "in_legacy_2d_tv": dict(kind="in", weight2d=True, versioned=False, tv=True),
    "bn_var": dict(kind="bn"),
    "bn_std_legacy_2d": dict(kind="bn", running_std=True, weight2d=True, versioned=False),
    "bn_var_tv": dict(kind="bn", tv=True),
}


def make_file_bytes(variant, seed=0, out_scale=1.0):
    """-> (file bytes, the canonical parameters inside)."""
    v = dict(VARIANTS[variant])
    kind = v.pop("kind")
    P = make_params(kind, seed, out_scale)
    return dumps(build_tree(kind, P, **v)), P
