"""Record tests/golden/flow_blur_parent.npz: the bits that the Farneback flow, the motion alpha and the region feather
produced BEFORE csrc/ kept one Farneback, one separable blur (blur_ops.hip) and one set of border helpers
(border_common.h).  tests/test_gpu_flow.py and tests/test_gpu_regions.py compare the present library with it bit
for bit: nothing in these paths may change.

Run once on the GPU with NST_HIP_LIB pointing at a library built from the parent commit, never from the code under
test, and name that commit:

    NST_HIP_LIB=/path/to/parent/libnst_hip.so python tests/golden/make_golden_flow_blur.py --commit <id>

Only the float32 outputs are stored; the inputs are regenerated from the seeds below (the tests import them from
this file).  Cases:
  farneback_72x96   T.farneback, default parameters, morph_ref.texture_pair(72, 96, 3, -2): one pyramid level
                    survives (the resize path, the first matrix update from zero flow)
  farneback_33x47   the same at 33x47: no level survives, only the 3-tap sigma <= 0 table, odd sizes, the 5-pixel
                    border-scale bands nearly meet
  motion_alpha      T.motion_alpha at the pipeline's sigma 3 on a 10x12 flow: the blur's half-width 12 >= both
                    sizes, so an index reflects twice
  feather_45x80     nst_region_feather, 4 planes of 45x80, ks = 81: half-width 40 < 45, the widest the entry point
                    admits at that height
  feather_12x300    2 planes of 12x300, ks = 21: two 256-pixel row tiles, the second partial (the LDS halo across
                    the tile edge)
"""
from __future__ import annotations

import argparse
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(HERE, "flow_blur_parent.npz")
FARNEBACK_SIZES = ((72, 96), (33, 47))
FEATHER_CASES = {"feather_45x80": (4, 45, 80, 81, 31), "feather_12x300": (2, 12, 300, 21, 32)}  # k, h, w, ks, seed


def farneback_pair(h, w):
    import morph_ref as MR
    return MR.texture_pair(h, w, 3, -2)


def motion_flow():
    rng = np.random.default_rng(21)
    return ((rng.random((10, 12, 2)).astype(np.float32) - 0.5) * 24).astype(np.float32)  # |flow| / 8 spans 0 .. 1


def feather_input(name):
    """The planes and the fp32 taps (oracle gaussian_taps at OpenCV's default sigma for ks) of a feather case."""
    from oracle import flow_oracle as FO
    k, h, w, ks, seed = FEATHER_CASES[name]
    planes = np.random.default_rng(seed).random((k, h, w)).astype(np.float32)
    return planes, FO.gaussian_taps(ks, 0.0).astype(np.float32)


def gpu_farneback(h, w):
    import torch
    from neuralstyletransferv1_amd import temporal as T
    dev = torch.device("cuda", 0)
    prev, nxt = farneback_pair(h, w)
    return T.farneback(torch.from_numpy(prev).to(dev), torch.from_numpy(nxt).to(dev)).cpu().numpy()


def gpu_motion_alpha():
    import torch
    from neuralstyletransferv1_amd import temporal as T
    return T.motion_alpha(torch.from_numpy(motion_flow()).to(torch.device("cuda", 0)), 0.9).cpu().numpy()


def gpu_feather(name):
    import torch
    from neuralstyletransferv1_amd import _lib
    dev = torch.device("cuda", 0)
    planes, taps = feather_input(name)
    m = torch.from_numpy(planes).to(dev)
    scratch = torch.empty_like(m)
    k, h, w = planes.shape
    _lib.check(_lib.lib().nst_region_feather(m.data_ptr(), k, h, w, taps.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                             len(taps), scratch.data_ptr(), _lib.stream_ptr(dev)), "nst_region_feather")
    return m.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the parent commit the library in NST_HIP_LIB was built from")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    if not os.environ.get("NST_HIP_LIB"):
        raise SystemExit("set NST_HIP_LIB to a library built from the parent commit (never record the code under test)")
    from neuralstyletransferv1_amd import _lib
    out = {"parent_commit": np.array(args.commit), "nst_version": np.array(_lib.lib().nst_version().decode())}
    for h, w in FARNEBACK_SIZES:
        out[f"farneback_{h}x{w}"] = gpu_farneback(h, w)
    out["motion_alpha"] = gpu_motion_alpha()
    for name in FEATHER_CASES:
        out[name] = gpu_feather(name)
    for k, v in out.items():
        assert v.dtype.kind == "U" or (v.dtype == np.float32 and np.isfinite(v).all()), k
    np.savez(args.out, **out)
    print("wrote", args.out, {k: v.shape for k, v in out.items()}, "from", _lib.LIB_PATH)


if __name__ == "__main__":
    main()
