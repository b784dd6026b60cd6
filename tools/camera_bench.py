"""The morph slideshow's camera stage at the reference's default size (csrc/camera_ops.hip, camera.py; DESIGN.md
§7.4): a 72-frame transition to 720x1280 at --pan_zoom 2, i.e. the morph at 1440x2560, once with every effect on
(zoom pulse 0.05, hue rotation 90, temporal smoothing 3) and once with none (zoom-in and pan only).  One JSON line
per variant --

  morph_ms     optical_flow_morph at pan size (flows, post-processing, all 72 frames)
  camera_ms    nst_camera_frames_u8 over the 72 frames (three calls of at most 32 frames, two launches each), tables
               and descriptors prepared beforehand; prepare_host_ms is that host preparation (wall clock)
  smooth_ms    nst_camera_smooth_u8 over the 72 output frames (effects on only)
  *_floor_ms   the bytes the stage must move at the HBM rate a streaming kernel reaches on this part (6.3 TB/s):
               camera = every frame's patch read once + its output written once; smooth = every output frame read
               once and written once

each the median HIP-event time of --reps calls after --warmup calls, with the spread (min, max) and the compute clock
read before and after.  The CPU comparison is tests/camera_ref.py (the numpy restatement, not the reference's cv2)
on the same host at 144x256 -> 72x128, where the GPU stage is timed too: the restatement is too slow for the full
size.  No time is gated.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
HBM_BYTES_PER_S = 6.3e12
EFFECTS = {"all": dict(zoom_pulse=0.05, zoom_pulse_freq=2.0, hue_rotate=90.0, smooth=3),
           "none": dict(zoom_pulse=0.0, zoom_pulse_freq=2.0, hue_rotate=0.0, smooth=0)}


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


def _stage(frames, k, size, target, fx, warmup, reps):
    """The camera (and smoothing) times of k frames [k,h,w,3] on the device, with their floors."""
    from neuralstyletransferv1_amd import camera as CAM
    plan = CAM.frame_plan(k, size, target, 2.0, "horizontal", 0.25, fx["zoom_pulse"], fx["zoom_pulse_freq"],
                          fx["hue_rotate"])
    t0 = time.perf_counter()
    calls = CAM.prepare_camera(plan, target, frames.device)
    r = {"zoom_phase_frames": sum(p.zoom for p in plan), "prepare_host_ms": round((time.perf_counter() - t0) * 1e3, 2)}
    r["camera_ms"] = _timed(lambda: CAM.run_camera(frames, calls, target), warmup, reps)
    tw, th = target
    floor = sum(p.patch_w * p.patch_h * 3 + tw * th * 3 for p in plan) / HBM_BYTES_PER_S * 1e3
    r["camera_floor_ms"] = round(floor, 4)
    r["camera_x_floor"] = round(r["camera_ms"]["median"] / floor, 1)
    if fx["smooth"]:
        out = CAM.run_camera(frames, calls, target)
        r["smooth_ms"] = _timed(lambda: CAM.temporal_smooth_frames(out, fx["smooth"]), warmup, reps)
        floor = 2 * k * tw * th * 3 / HBM_BYTES_PER_S * 1e3
        r["smooth_floor_ms"] = round(floor, 4)
        r["smooth_x_floor"] = round(r["smooth_ms"]["median"] / floor, 1)
    return r, plan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=72)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no_cpu", action="store_true", help="skip the numpy restatement's timing")
    ap.add_argument("--out", default=None, help="also append the JSON lines here")
    args = ap.parse_args()
    import numpy as np
    import torch

    from neuralstyletransferv1_amd import morph as MO, synthetic
    if not torch.cuda.is_available():
        raise SystemExit("camera_bench: no GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    k = args.frames
    lines = []
    for name, fx in EFFECTS.items():
        res = {"tool": "camera_bench", "effects": name, **{a: b for a, b in fx.items()}, "frames": k, "pan_zoom": 2.0,
               "warmup": args.warmup, "reps": args.reps, "clock_before": _clock()}
        for tag, (tw, th) in (("720x1280", (720, 1280)), ("72x128", (72, 128))):
            w, h = 2 * tw, 2 * th
            st = synthetic.make_frames(2, h, w, seed=71)
            a, b = torch.from_numpy(st[0]).to(dev), torch.from_numpy(st[1]).to(dev)
            r = {"target_wh": [tw, th], "morph_wh": [w, h],
                 "morph_ms": _timed(lambda: MO.optical_flow_morph(a, b, k, "v2", "smooth"), args.warmup, args.reps)}
            frames = MO.optical_flow_morph(a, b, k, "v2", "smooth")
            stage, plan = _stage(frames, k, (w, h), (tw, th), fx, args.warmup, args.reps)
            r.update(stage)
            if tag == "72x128" and not args.no_cpu:
                import camera_ref as CR
                host = list(frames.cpu().numpy())
                t0 = time.perf_counter()
                CR.camera_sequence(host, [dict(p.__dict__) for p in plan], tw, th, fx["smooth"])
                r["numpy_restatement_ms_same_host"] = round((time.perf_counter() - t0) * 1e3, 1)
            del frames
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
