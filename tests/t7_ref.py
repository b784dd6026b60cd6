"""The tests' oracle for Torch7 fast-style files: a small generic interpreter of the parsed module tree in torch-CPU
fp32, with the reference's pre / post arithmetic around it (pipeline.py:445-478, 1443, 1512-1516).

It walks whatever modules the file holds and knows nothing of the expected architecture: it does not go through
torch7.match_network, so the engine's reading of a file and this one are independent.
"""
import numpy as np
import torch
import torch.nn.functional as F

from neuralstyletransferv1_amd import torch7 as T7


def _mods(m):
    t = m.get("modules")
    return [t[i] for i in range(1, len(t) + 1)]


def _f32(t):
    return t.to(torch.float32)


def run(m, x):
    """One module's forward (x: a tensor, or a list of tensors after nn.ConcatTable)."""
    cls = m.torch_class
    if cls == "nn.Sequential":
        for c in _mods(m):
            x = run(c, x)
        return x
    if cls == "nn.ConcatTable":
        return [run(c, x) for c in _mods(m)]
    if cls == "nn.CAddTable":
        y = x[0]
        for t in x[1:]:
            y = y + t
        return y
    if cls == "nn.SpatialReflectionPadding":
        return F.pad(x, tuple(int(m.get(k)) for k in ("pad_l", "pad_r", "pad_t", "pad_b")), mode="reflect")
    if cls in ("nn.SpatialConvolution", "nn.SpatialFullConvolution"):
        cin, cout = int(m.get("nInputPlane")), int(m.get("nOutputPlane"))
        kh, kw = int(m.get("kH")), int(m.get("kW"))
        stride = (int(m.get("dH", 1)), int(m.get("dW", 1)))
        pad = (int(m.get("padH", 0) or 0), int(m.get("padW", 0) or 0))
        b = _f32(m.get("bias"))
        if cls == "nn.SpatialConvolution":
            return F.conv2d(x, _f32(m.get("weight")).reshape(cout, cin, kh, kw), b, stride=stride, padding=pad)
        adj = (int(m.get("adjH", 0) or 0), int(m.get("adjW", 0) or 0))
        return F.conv_transpose2d(x, _f32(m.get("weight")).reshape(cin, cout, kh, kw), b, stride=stride, padding=pad,
                                  output_padding=adj)
    if cls == "nn.InstanceNormalization":
        return F.instance_norm(x, weight=_f32(m.get("weight")), bias=_f32(m.get("bias")), eps=float(m.get("eps")))
    if cls == "nn.SpatialBatchNormalization":
        eps = float(m.get("eps"))
        var = m.get("running_var")
        if not isinstance(var, torch.Tensor) or var.numel() == 0:  # legacy: running_std = 1 / sqrt(var + eps)
            std = m.get("running_std").double()
            var = (1.0 / (std * std) - eps).float()
        w = m.get("weight") if m.get("affine", True) else None
        b = m.get("bias") if m.get("affine", True) else None
        return F.batch_norm(x, _f32(m.get("running_mean")), _f32(var), None if w is None else _f32(w),
                            None if b is None else _f32(b), False, 0.0, eps)
    if cls == "nn.ReLU":
        return F.relu(x)
    if cls == "nn.Tanh":
        return torch.tanh(x)
    if cls == "nn.MulConstant":
        return x * float(m.get("constant_scalar"))
    if cls == "nn.ShaveImage":
        s = int(m.get("size"))
        return x[:, :, s:-s, s:-s]
    if cls == "nn.TotalVariation":
        return x
    raise NotImplementedError(cls)


def blob(frames_u8: np.ndarray) -> np.ndarray:
    """pipeline.py:450-463: uint8 RGB [n,h,w,3] -> the mean-subtracted BGR blob [n,3,h,w] float32."""
    bgr = np.ascontiguousarray(frames_u8[..., ::-1]).astype(np.float32)
    bgr[..., 0] -= 103.939
    bgr[..., 1] -= 116.779
    bgr[..., 2] -= 123.68
    return np.transpose(bgr, (0, 3, 1, 2)).copy()


def forward(root, x: np.ndarray) -> np.ndarray:
    """net.forward() of the reference: blob -> tanh(.) * constant, [n,3,oh,ow] float32."""
    with torch.no_grad():
        return run(root, torch.from_numpy(x)).numpy()


def frames_of(y: np.ndarray) -> np.ndarray:
    """pipeline.py:467-474: add the mean back, clip, truncate, BGR -> RGB: [n,oh,ow,3] uint8."""
    out = np.transpose(y, (0, 2, 3, 1)).copy()
    out[..., 0] += 103.939
    out[..., 1] += 116.779
    out[..., 2] += 123.68
    out = np.clip(out, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(out[..., ::-1])


def out01(root, frames_u8: np.ndarray, size=None) -> torch.Tensor:
    """What the reference hands on at :1443 / :1512-1516: to_tensor(pil_out).clamp(0, 1), fitted bilinearly to the
    content size `size` (default: the frames' own) when the net's output differs.  [n,3,h,w] float32."""
    fr = frames_of(forward(root, blob(frames_u8)))
    o = torch.from_numpy(fr).permute(0, 3, 1, 2).to(torch.float32).div(255).clamp(0, 1)
    size = tuple(size) if size is not None else tuple(frames_u8.shape[1:3])
    if tuple(o.shape[-2:]) != size:
        o = F.interpolate(o, size=size, mode="bilinear", align_corners=False)
    return o


def to_u8(o01: torch.Tensor) -> np.ndarray:
    """ToPILImage: pic.mul(255).byte() -> [n,h,w,3] uint8."""
    return o01.mul(255).byte().permute(0, 2, 3, 1).contiguous().numpy()


def stylize_u8(root, frames_u8: np.ndarray) -> np.ndarray:
    return to_u8(out01(root, frames_u8))


def saturated_fraction(frames: np.ndarray) -> float:
    return float(((frames == 0) | (frames == 255)).mean())


def load(data: bytes):
    return T7.read_t7_bytes(data)
