"""Generate tests/golden/deeplab_drn_*.npz from the REFERENCE DeepLab modules with backbone='drn' (build container
only; /root/reference does not exist on the GPU box and nothing at test time reads it).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_deeplab_drn.py

The reference's modeling/deeplab.py DeepLab(backbone='drn', output_stride=16, sync_bn=False) — what
sky_swap.py:160-166 load_deeplab builds for --backbone drn; deeplab.py:13-14 turns the output stride into 8 — is
instantiated with the DRN-D-54 download disabled exactly as sky_swap.py:53-72 disables it (model_zoo.load_url
returns {}), loaded strict=True with the seeded synthetic checkpoint (neuralstyletransferv1_amd/deeplab.py
make_state_dict(..., backbone="drn"), numpy PCG64) and run in eval mode on seeded inputs.  Stored: input x, logits
y, and a sha256 of the weights so a drifting generator is detected.

Cases (n = 1):
  * 33x47, 19 classes: odd extents 33 -> 17 -> 9 -> 5; on the 5x6 feature map every ASPP 3x3 keeps only its centre
    tap and layer6's dilation 4 is barely live.
  * 104x136, 21 classes: the 13x17 map makes dilation 12 live on both axes while 24 and 36 stay centre-only.
Each golden must leave the 16-bit GPU tests room under the 2 % of pixels they let disagree: at most 1 % of pixels
may have a top-2 margin <= 2 * 3e-2 * max|logit| (the bf16 bar's undecided band); the generator asserts it, so a
seed that fails it cannot be written.  Seeds: with make_state_dict's rules the class offsets of a random classifier
are as large as the logits' spatial variation, so that band (6 % of max|logit|) is only this empty where one class
wins almost everywhere — of seeds 0..259 at 104x136 with 21 classes, 101 (0.08 %), 255, 195, 203 and 135 pass, each
with one class on > 99 % of the pixels; seed 0 passes at 33x47 with 19 classes (0.64 %).  Inputs with large flat
regions spread the classes out but leave 20-80 % of the pixels inside the band.  The logit bars are what pins the
network; the argmax checks add the near-tie logic.

The 104x136 logits (1.19 MB of fp32) do not fit the repository's 1 MiB limit for a committed file as a plain
array, so a `y` that would not fit is stored losslessly as `y_dplanes`: the uint32 patterns differenced along H
(mod 2^32), split into their four byte planes (smooth logits make the high planes nearly constant);
tests/drn_ref.py load_golden undoes it bit-exactly, and the generator checks the round trip.
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("NST_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)

from neuralstyletransferv1_amd import deeplab  # noqa: E402

CASES = [
    # seed, num_classes, n, h, w
    (0, 19, 1, 33, 47),
    (101, 21, 1, 104, 136),
]
MAX_FILE_BYTES = 1 << 20
BF16_LOGIT_REL = 3e-2      # tests/test_gpu_deeplab_drn.py LOGIT_REL["bf16"]
UNDECIDED_MAX = 0.01


def weights_sha(sd) -> str:
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.numpy().tobytes())
    return h.hexdigest()


def ref_deeplab(num_classes: int):
    import torch.utils.model_zoo as model_zoo
    model_zoo.load_url = lambda *a, **k: {}  # sky_swap.py:53-72: no backbone download
    sys.path.insert(0, REF)
    try:
        from modeling.deeplab import DeepLab
        return DeepLab(num_classes=num_classes, backbone="drn", output_stride=16, sync_bn=False, freeze_bn=False)
    finally:
        sys.path.remove(REF)


def undecided_share(y: np.ndarray) -> float:
    s = np.sort(y, axis=1)
    margin = s[:, -1] - s[:, -2]
    return float((margin <= 2 * BF16_LOGIT_REL * np.abs(y).max()).mean())


def encode_dplanes(y: np.ndarray) -> np.ndarray:
    """fp32 [n, c, h, w] -> uint8 [4, n*c*h*w]: byte planes of the bit patterns' differences along H."""
    d = np.diff(np.ascontiguousarray(y).view(np.uint32), axis=-2, prepend=np.uint32(0)).astype(np.uint32)
    return np.ascontiguousarray(d.view(np.uint8).reshape(-1, 4).T)


def main():
    torch.set_num_threads(8)
    for seed, nc, n, h, w in CASES:
        sd = deeplab.make_state_dict(nc, seed, backbone="drn")
        m = ref_deeplab(nc)
        assert list(m.state_dict()) == list(sd), "DRN skeleton keys / order differ from the reference module's"
        assert all(tuple(v.shape) == tuple(sd[k].shape) for k, v in m.state_dict().items())
        m.load_state_dict(sd, strict=True)
        m.eval()
        g = torch.Generator().manual_seed(100 + seed)
        x = torch.randn((n, 3, h, w), generator=g) * 1.2
        with torch.no_grad():
            y = m(x)
        und = undecided_share(y.numpy())
        print(f"seed {seed} {h}x{w} nc={nc}: {len(sd)} tensors, max|y| {float(y.abs().max()):.4f}, std "
              f"{float(y.std()):.4f}, classes used {len(np.unique(y.argmax(1).numpy()))}, undecided under the bf16 bar "
              f"{100 * und:.2f} %")
        assert und <= UNDECIDED_MAX, (seed, h, w, und)
        path = os.path.join(HERE, f"deeplab_drn_s{seed}_{h}x{w}.npz")
        meta = dict(x=x.numpy(), seed=seed, num_classes=nc, weights_sha256=weights_sha(sd),
                    torch_version=torch.__version__)
        np.savez_compressed(path, y=y.numpy(), **meta)
        if os.path.getsize(path) > MAX_FILE_BYTES:
            np.savez_compressed(path, y_dplanes=encode_dplanes(y.numpy()), **meta)
        sys.path.insert(0, os.path.dirname(HERE))
        from drn_ref import load_golden
        assert np.array_equal(load_golden(path)["y"].view(np.uint32), y.numpy().view(np.uint32))
        assert os.path.getsize(path) <= MAX_FILE_BYTES, os.path.getsize(path)
        print(path, tuple(y.shape), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
