"""Multi-model video at the workload's 1080x1920 portrait (csrc/multi_model_ops.hip): one JSON line
per size for the default chain (styled 17..160 of 176 source frames, a 48-frame cross-fade, 3 hold frames; udnie
ladder of 5 rungs, mosaic, tenharmsel) as multi_model_video.plan() emits it with every file in place --

  styled    32 frames from the middle of the styled section: the ramped base, both overlays, the saturation boost
  faded     the section's first 16 frames (the fade-in from the original) and its last 16 (the cross-fade out)
  intro     the 16 intro frames: a plain original cross-fading into the udnie still

each frame reading its own images (a batch's bank is the frames' file lists one after the other, as the CLI builds
it) --

  kernel_ms      nst_multi_model_frames over the pre-packed descriptors (groups of 8 frames per launch)
  call_ms        multi_model_video.multi_model_frames: the same with the descriptors packed per call and the output
                 allocated
  images_per_frame, gb_per_s   every image a frame names read once and the frame written once, over kernel_ms

and the yardstick in the same session: nst_style_morph_frames at the same pixel count over 32 frames that read 7
images each (the original and three families' two rungs, the saturation filter), accounted the same way.  Each figure
is the median HIP-event time of --reps calls after --warmup calls, with the spread (min, max) over --rounds rounds
that alternate the kernel with its yardstick, and the compute clock read before and after.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
WEIGHTS = {"udnie": [f"udnie_style{v}" for v in ("5e10", "1e11", "5e11", "1e12", "5e12")],
           "tenharmsel": [f"tenharmsel_style{v}" for v in ("1e9", "5e9", "1e10", "5e10", "1e11", "5e11")]}
TOTAL, START, END, CROSSFADE, HOLD = 176, 17, 160, 48, 3


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


def _summary(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def workloads(MM):
    """{name: (descriptors over one concatenated bank, images in that bank)} from plan() with every file in place."""
    dirs = {k: Path("/bench") / k for k in ("udnie", "mosaic", "tenharmsel")}
    pl = MM.plan(Path("/bench/orig"), dirs, WEIGHTS, TOTAL, lambda p: True, None, START, END, CROSSFADE, HOLD, 0.4, 1.3)
    by_frame = {fr["frame"]: fr for fr in pl}
    mid = (START + END) // 2
    picks = {"styled": range(mid - 16, mid + 16), "faded": list(range(START, START + 16)) + list(range(END - 15, END + 1)),
             "intro": range(1, START)}
    out = {}
    for name, frames in picks.items():
        descs, n_bank = [], 0
        for f in frames:
            descs.append(MM.shifted(by_frame[f]["desc"], n_bank))
            n_bank += len(by_frame[f]["files"])
        out[name] = (descs, n_bank)
    return out


def yardstick(SM, n):
    """n style-morph descriptors reading 7 images each (the original, three two-rung families), saturation filter."""
    code, fparam = SM.FILTER_PARAMS["subtle_sat"]
    descs = []
    for i in range(n):
        b = 7 * i
        terms = [dict(lo=b + 1 + 2 * t, hi=b + 2 + 2 * t, w_lo=0.6, w_hi=0.4, weight=0.2) for t in range(3)]
        descs.append(dict(n_sides=1, fade=(1.0, 0.0), sides=[dict(orig=b, orig_w=0.4, terms=terms)], filter=code,
                          fparam=fparam))
    return descs, 7 * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the kernel and its yardstick")
    ap.add_argument("--sizes", type=str, default="1920x1080,240x135", help="HxW list")
    ap.add_argument("--out", default=None, help="also append the JSON lines here")
    args = ap.parse_args()
    import torch

    from neuralstyletransferv1_amd import _lib, multi_model_video as MM, style_morph as SM
    if not torch.cuda.is_available():
        raise SystemExit("multi_model_bench: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    loads = workloads(MM)
    lines = []
    for size in args.sizes.split(","):
        h, w = (int(v) for v in size.split("x"))
        fbytes = h * w * 3
        res = {"tool": "multi_model_bench", "hw": [h, w], "warmup": args.warmup, "reps": args.reps,
               "rounds": args.rounds, "clock_before": _clock()}
        gen = torch.Generator(device=dev).manual_seed(81)
        descs_y, n_bank_y = yardstick(SM, 32)
        bank_y = torch.randint(0, 256, (n_bank_y, h, w, 3), dtype=torch.uint8, device=dev, generator=gen)
        out_y = torch.empty((len(descs_y), h, w, 3), dtype=torch.uint8, device=dev)
        packed_y = SM.pack(descs_y)

        def morph():
            _lib.check(lib.nst_style_morph_frames(bank_y.data_ptr(), n_bank_y, h, w, packed_y, len(descs_y),
                                                  out_y.data_ptr(), _lib.stream_ptr(dev)), "nst_style_morph_frames")

        yms = []
        for tag, (descs, n_bank) in loads.items():
            n = len(descs)
            bank = torch.randint(0, 256, (n_bank, h, w, 3), dtype=torch.uint8, device=dev, generator=gen)
            out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
            packed = MM.pack(descs)

            def kernel():
                _lib.check(lib.nst_multi_model_frames(bank.data_ptr(), n_bank, h, w, packed, n, out.data_ptr(),
                                                      _lib.stream_ptr(dev)), "nst_multi_model_frames")

            kms, cms = [], []
            for _ in range(args.rounds):
                kms += _times(kernel, args.warmup, args.reps)
                cms += _times(lambda: MM.multi_model_frames(bank, descs), args.warmup, args.reps)
                yms += _times(morph, args.warmup, args.reps)
            moved = (n_bank + n) * fbytes
            k = _summary(kms)
            res[tag] = {"frames": n, "images_per_frame": round(n_bank / n, 2), "kernel_ms": k, "call_ms": _summary(cms),
                        "ms_per_frame": round(k["median"] / n, 5), "gb_per_s": round(moved / k["median"] / 1e6, 1),
                        "gb_per_s_spread": [round(moved / k["max"] / 1e6, 1), round(moved / k["min"] / 1e6, 1)]}
            del bank, out
        k = _summary(yms)
        moved = (n_bank_y + len(descs_y)) * fbytes
        res["style_morph_yardstick"] = {"frames": len(descs_y), "images_per_frame": 7.0, "kernel_ms": k,
                                        "gb_per_s": round(moved / k["median"] / 1e6, 1),
                                        "gb_per_s_spread": [round(moved / k["max"] / 1e6, 1),
                                                            round(moved / k["min"] / 1e6, 1)]}
        del bank_y, out_y
        res["clock_after"] = _clock()
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
