"""Optical-flow morph at 1080p (csrc/morph_ops.hip, the Gaussian-window Farneback of csrc/flow_ops.hip; DESIGN.md
§7.4): one JSON line per preset for a transition of 72 frames between two 1080p stills --

  flows_ms    grey (+ pre-blur for v2) and the forward and backward Farneback flows (nst_flow_farneback_ex, n = 2)
  post_ms     nst_morph_flow_post (v2 only)
  frames_ms   one nst_morph_frames launch writing all 72 frames, and that as a multiple of its write floor
              k * h * w * 3 bytes / the HBM rate a streaming kernel reaches on this part (6.3 TB/s, of 8 TB/s spec)

each the median HIP-event time of --reps calls after --warmup calls, with the spread (min, max) and the compute
clock read before and after.  The CPU comparison is tests/morph_ref.py (the numpy restatement, not the reference's
cv2) on the same host at 270x480, where the GPU transition is timed too: the restatement is too slow for 1080p.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
HBM_BYTES_PER_S = 6.3e12


def _clock():
    """The compute clock line of GPU 0 as rocm-smi shows it (read only), or a note that it could not be read."""
    try:
        out = subprocess.run(["rocm-smi", "-d", "0", "-c"], capture_output=True, text=True, timeout=20).stdout
        lines = [l.strip() for l in out.splitlines() if "sclk" in l]
        return lines[0] if lines else "not read"
    except Exception as e:  # the measurement stands without it
        return f"not read ({type(e).__name__})"


def _timed(fn, warmup, reps):
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
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=72)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no_cpu", action="store_true", help="skip the numpy restatement's timing")
    ap.add_argument("--out", default=None, help="also append the JSON lines here")
    args = ap.parse_args()
    import torch

    from neuralstyletransferv1_amd import _lib, morph as MO, synthetic
    if not torch.cuda.is_available():
        raise SystemExit("morph_bench: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    k = args.frames
    lines = []
    for preset in ("slideshow", "v2"):
        p = MO.PRESETS[preset]
        res = {"tool": "morph_bench", "preset": preset, "frames": k, "warmup": args.warmup, "reps": args.reps,
               "clock_before": _clock()}
        for tag, (h, w) in (("1080p", (1080, 1920)), ("270x480", (270, 480))):
            st = synthetic.make_frames(2, h, w, seed=70)
            a, b = torch.from_numpy(st[0]).to(dev), torch.from_numpy(st[1]).to(dev)
            t, alpha = MO.schedule(k, preset, "smooth")

            def flows():
                g = MO.gray_cv_u8(torch.stack([a, b]))
                if p["pre_blur"]:
                    g = MO.gauss_u8(g)
                return MO.farneback_ex(g, g.flip(0), p["farneback"], _lib.NST_FLOW_GAUSSIAN)

            raw = flows()
            fl = MO.flow_post(raw, (1.0, -1.0)) if p["post"] else raw
            r = {"hw": [h, w], "flows_ms": _timed(flows, args.warmup, args.reps)}
            if p["post"]:
                r["post_ms"] = _timed(lambda: MO.flow_post(raw, (1.0, -1.0)), args.warmup, args.reps)
            r["frames_ms"] = _timed(lambda: MO.morph_frames(a, b, fl[0], fl[1], t, alpha), args.warmup, args.reps)
            floor_ms = k * h * w * 3 / HBM_BYTES_PER_S * 1e3
            r["frames_write_floor_ms"] = round(floor_ms, 4)
            r["frames_x_write_floor"] = round(r["frames_ms"]["median"] / floor_ms, 2)
            r["transition_ms"] = _timed(lambda: MO.optical_flow_morph(a, b, k, preset, "smooth"), args.warmup, args.reps)
            if tag == "270x480" and not args.no_cpu:
                import morph_ref as MR
                t0 = time.perf_counter()
                MR.optical_flow_morph(st[0], st[1], k, preset, "smooth")
                r["numpy_restatement_ms_same_host"] = round((time.perf_counter() - t0) * 1e3, 1)
            res[tag] = r
        res["clock_after"] = _clock()
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
