"""CPU restatement of the DRN-D-54 DeepLab v3+ forward (modeling/deeplab.py:27-33 with backbone='drn') from a state
dict — TEST INFRASTRUCTURE ONLY, the checker of tests/test_deeplab_drn_host.py and tests/test_gpu_deeplab_drn.py.

PyTorch-CPU fp32 functional ops in the reference modules' own order (drn.py:208-234 DRN.forward with Bottleneck
:79-99, aspp.py:65-78 at output stride 8, decoder.py:34-43, BatchNorm2d in eval mode), pinned bit-exact against the
reference modules by tests/golden/deeplab_drn_*.npz (tests/golden/make_golden_deeplab_drn.py).  The mask chain
around it (preprocess, LANCZOS, post-processing, INTER_LINEAR) is oracle/deeplab_oracle.py's, unchanged."""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from oracle.deeplab_oracle import cv_resize_linear_u8, infer_post, lanczos, preprocess_u8

# drn.py:386-387 drn_d_54: blocks per bottleneck layer 3..6 and (stride of block 0, dilation of every conv2)
BLOCKS = {3: (3, 2, 1), 4: (4, 2, 1), 5: (6, 1, 2), 6: (3, 1, 4)}
ASPP_DILATIONS = (1, 12, 24, 36)  # aspp.py:45-46, output stride 8 (deeplab.py:13-14 forces it for drn)


def load_golden(path: str) -> dict:
    """A tests/golden/deeplab_drn_*.npz as a dict with the reference logits under "y": stored plainly, or (a file
    that would pass 1 MiB otherwise) as "y_dplanes" — the four byte planes of the fp32 bit patterns differenced
    along H, undone here bit-exactly (tests/golden/make_golden_deeplab_drn.py encode_dplanes)."""
    z = dict(np.load(path))
    if "y" not in z:
        x = z["x"]
        shape = (x.shape[0], int(z["num_classes"]), x.shape[2], x.shape[3])
        d = np.ascontiguousarray(z.pop("y_dplanes").T).view(np.uint32).reshape(shape)
        z["y"] = np.cumsum(d, axis=-2, dtype=np.uint32).view(np.float32)
    return z


def _bn(sd: Dict[str, torch.Tensor], pre: str, x: torch.Tensor) -> torch.Tensor:
    return F.batch_norm(x, sd[pre + ".running_mean"], sd[pre + ".running_var"], sd[pre + ".weight"], sd[pre + ".bias"],
                        False, 0.1, 1e-5)


def _conv_layer(sd, pre: str, x: torch.Tensor, stride: int, dilation: int, padding: int) -> torch.Tensor:
    """One Conv2d + BatchNorm + ReLU of layer0 / _make_conv_layers (drn.py:124-129, :196-206)."""
    return F.relu(_bn(sd, pre + ".1", F.conv2d(x, sd[pre + ".0.weight"], stride=stride, padding=padding,
                                               dilation=dilation)))


def _bottleneck(sd, pre: str, x: torch.Tensor, stride: int, dilation: int, has_ds: bool) -> torch.Tensor:
    """drn.py:79-99 (conv2 carries the stride and dilation[1])."""
    out = F.relu(_bn(sd, pre + ".bn1", F.conv2d(x, sd[pre + ".conv1.weight"])))
    out = F.relu(_bn(sd, pre + ".bn2", F.conv2d(out, sd[pre + ".conv2.weight"], stride=stride, padding=dilation,
                                                dilation=dilation)))
    out = _bn(sd, pre + ".bn3", F.conv2d(out, sd[pre + ".conv3.weight"]))
    residual = _bn(sd, pre + ".downsample.1", F.conv2d(x, sd[pre + ".downsample.0.weight"], stride=stride)) if has_ds else x
    out += residual
    return F.relu(out)


def backbone(sd, x: torch.Tensor):
    """drn.py:208-234 for arch 'D': -> (features at 1/8 with 512 channels, layer3's output at 1/4 with 256)."""
    x = _conv_layer(sd, "backbone.layer0", x, 1, 1, 3)
    x = _conv_layer(sd, "backbone.layer1", x, 1, 1, 1)
    x = _conv_layer(sd, "backbone.layer2", x, 2, 1, 1)
    low = None
    for li in (3, 4, 5, 6):
        nb, stride, dil = BLOCKS[li]
        for i in range(nb):
            x = _bottleneck(sd, f"backbone.layer{li}.{i}", x, stride if i == 0 else 1, dil, i == 0)
        if li == 3:
            low = x
    x = _conv_layer(sd, "backbone.layer7", x, 1, 2, 2)
    x = _conv_layer(sd, "backbone.layer8", x, 1, 1, 1)
    return x, low


def aspp(sd, x: torch.Tensor) -> torch.Tensor:
    """aspp.py:65-78 (Dropout is the identity in eval)."""
    xs = []
    for i, d in enumerate(ASPP_DILATIONS):
        pre = f"aspp.aspp{i + 1}"
        pad = 0 if i == 0 else d
        xs.append(F.relu(_bn(sd, pre + ".bn", F.conv2d(x, sd[pre + ".atrous_conv.weight"], padding=pad, dilation=d))))
    x5 = F.adaptive_avg_pool2d(x, (1, 1))
    x5 = F.relu(_bn(sd, "aspp.global_avg_pool.2", F.conv2d(x5, sd["aspp.global_avg_pool.1.weight"])))
    x5 = F.interpolate(x5, size=xs[3].size()[2:], mode="bilinear", align_corners=True)
    x = torch.cat(xs + [x5], dim=1)
    return F.relu(_bn(sd, "aspp.bn1", F.conv2d(x, sd["aspp.conv1.weight"])))


def decoder(sd, x: torch.Tensor, low: torch.Tensor) -> torch.Tensor:
    """decoder.py:34-43."""
    low = F.relu(_bn(sd, "decoder.bn1", F.conv2d(low, sd["decoder.conv1.weight"])))
    x = F.interpolate(x, size=low.size()[2:], mode="bilinear", align_corners=True)
    x = torch.cat((x, low), dim=1)
    x = F.relu(_bn(sd, "decoder.last_conv.1", F.conv2d(x, sd["decoder.last_conv.0.weight"], padding=1)))
    x = F.relu(_bn(sd, "decoder.last_conv.5", F.conv2d(x, sd["decoder.last_conv.4.weight"], padding=1)))
    return F.conv2d(x, sd["decoder.last_conv.8.weight"], sd["decoder.last_conv.8.bias"])


@torch.no_grad()
def forward(sd: Dict[str, torch.Tensor], x: torch.Tensor) -> torch.Tensor:
    """deeplab.py:27-33: logits [n, nc, h, w]."""
    feat, low = backbone(sd, x)
    y = decoder(sd, aspp(sd, feat), low)
    return F.interpolate(y, size=x.size()[2:], mode="bilinear", align_corners=True)


def masks_from_frames(sd, frames: np.ndarray, target_ids: Sequence[int], resolution: int = 256, expand_px: int = 0,
                      contract_px: int = 0, feather_px: int = 3):
    """batch_masks_from_frames (sky_swap.py:286-362) for in-memory frames with the DRN network: -> (masks [n,H,W],
    preds [n,h,w], logits [n,nc,h,w]) at the working size h x w (the chain of deeplab_oracle.masks_from_frames)."""
    masks, preds, logits = [], [], []
    for f in frames:
        H, W = f.shape[:2]
        w, h = W, H
        if resolution and resolution > 0:
            scale = float(resolution) / max(W, H)
            if scale < 1.0:
                w, h = int(W * scale), int(H * scale)
        work = f if (w, h) == (W, H) else lanczos(f, w, h)
        lg = forward(sd, preprocess_u8(work))
        pred = lg.argmax(1).squeeze(0).numpy().astype(np.uint8)
        m = infer_post(pred, target_ids, expand_px, contract_px, feather_px)
        if (w, h) != (W, H):
            m = cv_resize_linear_u8(m, W, H)
        masks.append(m)
        preds.append(pred)
        logits.append(lg[0].numpy())
    return np.stack(masks), np.stack(preds), np.stack(logits)
