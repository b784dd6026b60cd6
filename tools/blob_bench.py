"""The soft-blob compositor at the reference's sizes (csrc/blob_ops.hip): one JSON line with, per frame
size (1440x1080, 1280x720) and blob count (2, 4, 8), over 16 consecutive frames of selfstyle_blob.plan() on a bank of
24 random stills (two launches of 8 frames) --

  kernel_ms      nst_blob_frames over the pre-packed field and descriptors, per frame
  call_ms        selfstyle_blob.blob_frames: the same with the structs packed per call and the output allocated, per frame
  masks_ms       nst_blob_masks for the same frames, per frame (the noise field and the softmax without the stills)
  gsin_per_s     diagonal sines per second over kernel_ms (4 per pixel and blob; the row and column terms come on top)

Each figure is the median HIP-event time of --reps calls after --warmup calls, with the spread (min, max) over
--rounds rounds, and the compute clock read before and after.  There is no CPU path to time.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
N_FRAMES, N_STILLS, FIRST = 16, 24, 352


def _clock():
    """The compute clock line of GPU 0 as rocm-smi shows it (read only), or a note that it could not be read."""
    try:
        out = subprocess.run(["rocm-smi", "-d", "0", "-c"], capture_output=True, text=True, timeout=20).stdout
        lines = [l.strip() for l in out.splitlines() if "sclk" in l]
        return lines[0] if lines else "not read"
    except Exception as e:  # the measurement stands without it
        return f"not read ({type(e).__name__})"


def _times(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def _per_frame(ms):
    return {"median": round(statistics.median(ms) / N_FRAMES, 4), "min": round(min(ms) / N_FRAMES, 4),
            "max": round(max(ms) / N_FRAMES, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=str, default="1440x1080,1280x720", help="HxW list")
    ap.add_argument("--blobs", type=str, default="2,4,8")
    ap.add_argument("--out", default=None, help="also append the JSON line here")
    args = ap.parse_args()
    import torch

    from neuralstyletransferv1_amd import _lib, selfstyle_blob as SB
    if not torch.cuda.is_available():
        raise SystemExit("blob_bench: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    lib, st = _lib.lib(), _lib.stream_ptr(dev)
    res = {"tool": "blob_bench", "frames": N_FRAMES, "stills": N_STILLS, "warmup": args.warmup, "reps": args.reps,
           "rounds": args.rounds, "clock_before": _clock()}
    gen = torch.Generator(device=dev).manual_seed(83)
    for size in args.sizes.split(","):
        h, w = (int(v) for v in size.split("x"))
        bank = torch.randint(0, 256, (N_STILLS, h, w, 3), dtype=torch.uint8, device=dev, generator=gen)
        out = torch.empty((N_FRAMES, h, w, 3), dtype=torch.uint8, device=dev)
        yn, xn = SB.norm_tables(h, w, dev)
        for nb in (int(v) for v in args.blobs.split(",")):
            fd = SB.field(nb)
            descs = SB.plan(N_STILLS, 0, 24, 30, nb)[FIRST:FIRST + N_FRAMES]
            fld, packed = SB.pack_field(fd), SB.pack(descs)
            mout = torch.empty((N_FRAMES, nb, h, w), dtype=torch.float32, device=dev)

            def kernel():
                _lib.check(lib.nst_blob_frames(bank.data_ptr(), N_STILLS, h, w, yn.data_ptr(), xn.data_ptr(), fld, packed,
                                               N_FRAMES, out.data_ptr(), st), "nst_blob_frames")

            def masks():
                _lib.check(lib.nst_blob_masks(h, w, yn.data_ptr(), xn.data_ptr(), fld, packed, N_FRAMES, mout.data_ptr(),
                                              st), "nst_blob_masks")

            kms, cms, mms = [], [], []
            for _ in range(args.rounds):
                kms += _times(kernel, args.warmup, args.reps)
                cms += _times(lambda: SB.blob_frames(bank, yn, xn, fd, descs), args.warmup, args.reps)
                mms += _times(masks, args.warmup, args.reps)
            k = _per_frame(kms)
            res[f"{h}x{w}_b{nb}"] = {"kernel_ms": k, "call_ms": _per_frame(cms), "masks_ms": _per_frame(mms),
                                     "gsin_per_s": round(4 * nb * h * w / k["median"] / 1e6, 1)}
            del mout
        del bank, out
    res["clock_after"] = _clock()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
