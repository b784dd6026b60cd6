#!/usr/bin/env python3
"""pipeline.py — drop-in for the reference's CLI (pipeline.py:2156-2671) on the MI355X engine.

Same flags, defaults and modes (single image / batch images / video) as the reference; the
per-frame loop (`style_frames`, pipeline.py:527-2122, standard path :1409-1519 + post chain
:1881-2119) runs batched on the GPU:

    host: PIL decode (thread pool) -> uint8 frames --H2D--> [GPU] preset encode + net forward +
    decode + clamp + ToPILImage truncation (one nst_forward per model slot) -> multi-model blend
    -> LAB EMA (LUT, frame order) -> mask composite -> uniform blend --D2H--> host: PIL encode.

Additions: --gpus N (frames round-robin over N GPUs, ordered gather to rank 0 over RCCL),
--batch B (frames per GPU step), --dtype {fp32,fp32s,fp16m,bf16,fp16} (fp32 = parity with the reference's
arithmetic, default; fp32s = fp32 activations on split-fp16 MFMAs, the parity bar at several times
fp32's speed; fp16m = split-fp16 on the layers whose rounding reaches the frame, fp16 elsewhere: +-1 LSB
at most of the fp16 rate; bf16 = throughput mode; fp16 = near bf16's speed with 3 more mantissa bits),
--synthetic WxH / --synthetic_frames N (an
in-memory synthetic frame stream instead of files; config 4 of BASELINE.json).

Also on the GPU: the LAB multi-model blend (--blend_models_lab, pipeline.py:1841-1870) and the
Gaussian mask feather (--mask_feather / --mask_feather_pct, pipeline.py:349-351; cv2's blur
restated, parity unpinned because cv2 is absent here).

Region blending (--region_mode / --region_optimize and their spec, animation and rotation flags,
pipeline.py:1120-1407, 1720-1839) runs on the GPU compositor of regions.py.

The flow-guided EMA (--flow_ema with --flow_method dis, the default, or farneback, pipeline.py:1884-1940; any
--flow_downscale factor, floored like the reference's (W0 // ds, H0 // ds)) and the motion-adaptive blend
(--motion_blend, :2072-2086) run on the GPU (temporal.py).

Torch7 .t7 networks (--model_type torch7, or a .t7 file in any slot; pipeline.py:445-478, 583-596 runs them
through OpenCV DNN on the CPU) run on the engine (torch7.py); the half-size retry after a crashed OpenCV forward
(:1432-1442) is not imitated.

Not built (rejected with a clear message if requested): the Magenta (TF-Hub) backend.
"""
from __future__ import annotations

import argparse
import glob
import os
import re
import shutil
import subprocess
import sys
import time
import uuid
from concurrent.futures import ThreadPoolExecutor
from datetime import timedelta
from pathlib import Path
from typing import Dict, List, Optional

from . import frame_loop
# the frame loop's parts live in frame_loop.py; these names stay this module's too (tests, tools, regions.py)
from .frame_loop import FrameSource, _get_image_with_exif_pil, _log, load_mask_fit, load_mask_u8, parse_wh  # noqa: F401

IO_PRESETS_AUTO = {  # pipeline.py:2518-2523
    "transformer": "imagenet_255",
    "torch7": "caffe_bgr",
    "magenta": "imagenet_01",
    "reconet": "imagenet_01",
}
SLOTS = ["b", "c", "d", "e", "f", "g", "h"]


# the last style_frames run on this process: frames, seconds of the frame loop (decode -> GPU -> encode, from the
# first frame load to the last file written) and seconds of setup before it (model load, plans, size scan)
LAST_RUN_STATS: Dict[str, float] = {}


# ----------------------------------------------------------------------------- argparse
def build_parser() -> argparse.ArgumentParser:
    """Flag-for-flag mirror of pipeline.py:2157-2410 (+ engine flags at the end)."""
    ap = argparse.ArgumentParser(description="Extract -> Style -> Assemble (with temporal smoothing) on MI355X")
    ap.add_argument("--input_video", default=None)
    ap.add_argument("--output_video", default=None)
    ap.add_argument("--model", required=False)
    ap.add_argument("--work_dir", default="./_work")
    ap.add_argument("--fps", type=int, default=None)
    ap.add_argument("--pre_fps", type=int, default=None)
    ap.add_argument("--scale", type=int, default=None)
    ap.add_argument("--canvas", type=str, default=None)
    ap.add_argument("--image_ext", choices=["png", "jpg"], default="png")
    ap.add_argument("--jpeg_quality", type=int, default=85)
    ap.add_argument("--threads", type=int, default=4, help="host threads for frame decode/encode")
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--max_frames", type=int, default=None)
    ap.add_argument("--device", choices=["cpu", "mps", "cuda"], default="cuda")
    ap.add_argument("--gpu_memory_limit", type=int, default=32000)
    ap.add_argument("--inference_res", type=int, default=0)
    ap.add_argument("--io_preset", choices=["auto", "imagenet_255", "imagenet_01", "tanh", "caffe_bgr", "raw_255", "raw_01"],
                    default="auto")
    ap.add_argument("--input_image", type=str)
    ap.add_argument("--output_image", type=str)
    ap.add_argument("--input_dir", type=str)
    ap.add_argument("--output_dir", type=str)
    ap.add_argument("--pattern", type=str, default=None)
    ap.add_argument("--keep_ext", action="store_true")
    ap.add_argument("--output_suffix", type=str, default="")
    ap.add_argument("--output_prefix", type=str, default="styled_frame")
    ap.add_argument("--smooth_lightness", action="store_true", default=True)
    ap.add_argument("--no-smooth_lightness", action="store_false", dest="smooth_lightness")
    ap.add_argument("--smooth_alpha", type=float, default=0.7)
    ap.add_argument("--smooth_chroma", action="store_true", default=False)
    ap.add_argument("--chroma_alpha", type=float, default=0.85)
    ap.add_argument("--blend", type=float, default=1.0)
    ap.add_argument("--mask", type=str, default=None)
    ap.add_argument("--mask_invert", action="store_true")
    ap.add_argument("--mask_feather", type=int, default=0)
    ap.add_argument("--mask_dir", type=str, default=None)
    ap.add_argument("--mask_feather_pct", type=float, default=0.0)
    ap.add_argument("--mask_autofix", action="store_true", default=True)
    ap.add_argument("--mask_force_transpose", action="store_true")
    ap.add_argument("--mask_debug_overlay", action="store_true")
    ap.add_argument("--mask_debug_alpha", action="store_true")
    ap.add_argument("--fit_mask_to", choices=["input", "output"], default="input")
    ap.add_argument("--composite_mode", choices=["keep", "replace"], default="keep")
    ap.add_argument("--flow_ema", action="store_true", default=False)
    ap.add_argument("--flow_alpha", type=float, default=0.85)
    ap.add_argument("--flow_method", choices=["farneback", "dis"], default="dis")
    ap.add_argument("--flow_downscale", type=int, default=1)
    ap.add_argument("--model_type", choices=["transformer", "reconet", "magenta", "torch7"], default="transformer")
    for s in SLOTS:
        ap.add_argument(f"--model_{s}", type=str, default=None)
        ap.add_argument(f"--model_{s}_type", choices=["transformer", "reconet", "magenta", "torch7"], default=None)
        ap.add_argument(f"--io_preset_{s}", choices=["imagenet_255", "imagenet_01", "tanh", "caffe_bgr", "raw_255", "raw_01"],
                        default=None)
        ap.add_argument(f"--magenta_style_{s}", type=str, default=None)
    ap.add_argument("--blend_models_weights", type=str, default=None)
    ap.add_argument("--blend_models_lab", action="store_true")
    ap.add_argument("--blend_models_lab_weights", type=str, default=None)
    for flag, kw in (("--region_mode", dict(type=str, default=None, choices=["grid", "diagonal", "voronoi", "fractal",
                                                                           "radial", "waves", "spiral", "concentric",
                                                                           "random"])),
                     ("--region_count", dict(type=int, default=None)),
                     ("--region_sizes", dict(type=str, default=None)), ("--region_seed", dict(type=str, default=None)),
                     ("--region_feather", dict(type=int, default=20)),
                     ("--region_assignment", dict(type=str, default="random", choices=["sequential", "random", "weighted"])),
                     ("--region_original", dict(type=float, default=0.0)), ("--region_rotate", dict(type=float, default=0.0)),
                     ("--region_blend_spec", dict(type=str, default=None)), ("--region_scales", dict(type=str, default=None)),
                     ("--region_optimize", dict(action="store_true")), ("--region_padding", dict(type=int, default=64)),
                     ("--blend_animate", dict(type=str, default=None)), ("--blend_animate_regions", dict(type=str, default=None)),
                     ("--scale_animate", dict(type=str, default=None)), ("--scale_animate_regions", dict(type=str, default=None)),
                     ("--region_morph", dict(type=str, default=None))):
        ap.add_argument(flag, **kw)
    ap.add_argument("--magenta_style", type=str, default=None)
    ap.add_argument("--magenta_model_root", type=str, default="/app/models/magenta")
    ap.add_argument("--magenta_tile", type=int, default=256)
    ap.add_argument("--magenta_overlap", type=int, default=32)
    ap.add_argument("--magenta_target_res", type=int, default=None)
    ap.add_argument("--motion_blend", action="store_true")
    ap.add_argument("--clean_frames", action="store_true")
    ap.add_argument("--clean_work_dir", action="store_true")
    # ---- engine flags ----
    ap.add_argument("--gpus", type=int, default=int(os.environ.get("GPUS", "1")),
                    help="frames round-robin over N GPUs (one process per GPU), ordered gather to rank 0")
    ap.add_argument("--batch", type=int, default=8, help="frames per GPU per step")
    ap.add_argument("--dist_backend", choices=["nccl", "gloo"], default="nccl",
                    help="--gpus > 1 process group: nccl (RCCL over xGMI, one GPU per rank) or gloo (host-staged "
                         "exchange; ranks may share a GPU, used by the tests)")
    ap.add_argument("--dist_timeout", type=float, default=600.0, help="seconds before a blocked exchange aborts")
    ap.add_argument("--dtype", choices=["fp32", "fp32s", "fp16m", "bf16", "fp16"], default="fp32",
                    help="fp32 = parity with the reference arithmetic; fp32s = fp32 activations on split-fp16 "
                         "MFMAs (the same +-1 LSB parity, faster; conv inputs < 65504); fp16m = split-fp16 on the "
                         "first layers, fp16 elsewhere (+-1 LSB on 1080p frames, most of fp16's speed; ReCoNet runs "
                         "fp32s); bf16 = throughput mode; "
                         "fp16 = near the throughput mode's speed with 3 more mantissa bits (activations < 65504)")
    ap.add_argument("--synthetic", type=str, default=None, help="WxH: stylize an in-memory synthetic frame stream")
    ap.add_argument("--synthetic_frames", type=int, default=16)
    ap.add_argument("--no_save", action="store_true", help="do not encode/write outputs (throughput runs)")
    ap.add_argument("--keep_staged", action="store_true",
                    help="--input_dir: also write the staged frame copies (the reference's work_dir/frames files); the "
                         "frames are staged in memory either way, with the same pixels")
    ap.add_argument("--png_writer", choices=["fast", "pil", "gpu"], default="pil",
                    help="PNG outputs: 'pil' (default) = Pillow's encoder at its defaults, byte-identical to the "
                         "reference's files; 'fast' = Up filter + zlib RLE deflate (pngio.py: ~6x faster than Pillow's "
                         "default encoder, files within a few percent of its size, opt-in); 'gpu' = the whole file "
                         "built on the GPU that styled the frame (csrc/png_enc.hip: Up filter, per-scanline dynamic "
                         "Huffman blocks, CRC and Adler-32 on the device), the host only writes bytes.  The pixels are "
                         "identical either way")
    ap.add_argument("--jpeg_reader", choices=["pil", "gpu"], default="pil",
                    help="JPEG frames of the frame loop: 'pil' (default) = Pillow's decoder, as the reference; 'gpu' = "
                         "baseline JPEG files (what ffmpeg's mjpeg and Pillow write) are only entropy-decoded on the "
                         "host pool (csrc/jpeg_entropy.cpp) and rebuilt on the GPU (csrc/jpeg_dec.hip: IDCT, chroma "
                         "upsampling, colour conversion).  The pixels are Pillow's, byte for byte; any other file, a "
                         "damaged one, --inference_res and --input_dir staging keep Pillow")
    ap.add_argument("--jpeg_writer", choices=["pil", "gpu"], default="pil",
                    help="JPEG outputs: 'pil' (default) = Pillow's encoder at --jpeg_quality, as the reference; 'gpu' = "
                         "the whole file built on the GPU that styled the frame (csrc/jpeg_enc.hip: colour conversion, "
                         "4:2:0 downsampling, FDCT, quantisation, Huffman coding and 0xFF stuffing on the device), the "
                         "host only writes bytes.  The files are Pillow's, byte for byte; a --jpeg_quality outside "
                         "1..100 and a frame whose file outgrows the copied slot keep Pillow")
    ap.add_argument("--png_compress_level", type=int, default=None, choices=range(10), metavar="0-9",
                    help="Pillow's PNG encoder at this zlib level (overrides --png_writer); the pixels are the same "
                         "at every level, only the file size and the encode time change")
    return ap


def slot_model_type(args, s: str) -> str:
    """Back end of slot b..h: its own --model_<s>_type, else torch7 for a .t7 file, else slot A's (pipeline.py:631-632)."""
    p = getattr(args, f"model_{s}", None)
    auto = "torch7" if p and Path(str(p)).suffix.lower() == ".t7" else args.model_type
    return getattr(args, f"model_{s}_type", None) or auto


def reject_out_of_scope(args) -> None:
    bad = []
    if args.model_type == "magenta":
        bad.append(f"--model_type {args.model_type}")
    for s in SLOTS:
        if getattr(args, f"model_{s}") and (getattr(args, f"model_{s}_type") == "magenta"
                                             or str(getattr(args, f"model_{s}")).lower() in ("magenta",)):
            bad.append(f"--model_{s} (magenta)")
    if args.device != "cuda":
        bad.append(f"--device {args.device} (this engine runs on MI355X only; there is no CPU path)")
    if bad:
        _log("[error] not supported by the MI355X engine: " + ", ".join(bad))
        sys.exit(2)


# ----------------------------------------------------------------------------- host I/O helpers
def sh(cmd: str, check=True):
    _log(f"$ {cmd}")
    r = subprocess.run(cmd, shell=True)
    if check and r.returncode != 0:
        _log(f"[sh][ERROR] exit {r.returncode}")
        sys.exit(r.returncode)
    return r.returncode


def _require_ffmpeg():
    if shutil.which("ffmpeg") is None:
        _log("[error] video mode needs ffmpeg on PATH (frame extract/assemble, pipeline.py:384-419, 2128-2150)")
        sys.exit(2)


def extract_frames(input_video: Path, frames_dir: Path, fps, scale, img_ext: str, jpeg_quality: int, canvas_wh=None):
    """pipeline.py:384-419 (ffmpeg subprocess)."""
    _require_ffmpeg()
    frames_dir.mkdir(parents=True, exist_ok=True)
    vf = []
    if canvas_wh:
        cw, ch = canvas_wh
        vf.append(f"scale={cw}:{ch}:flags=lanczos:force_original_aspect_ratio=decrease")
        vf.append(f"pad={cw}:{ch}:(ow-iw)/2:(oh-ih)/2:color=black")
    elif scale:
        vf.append(f"scale='if(gte(iw,ih),{scale},-2)':'if(gte(ih,iw),{scale},-2)':flags=lanczos")
    if fps:
        vf.append(f"fps={fps}")
    ext = "png" if img_ext.lower() == "png" else "jpg"
    pattern = frames_dir / f"frame_%04d.{ext}"
    vfs = f'-vf "{",".join(vf)}" ' if vf else ""
    sh(f'ffmpeg -y -i "{input_video}" {vfs}-c:v mjpeg -q:v {jpeg_quality} -pix_fmt yuvj420p "{pattern}"')


def assemble_video(frames_dir: Path, output_video: Path, in_fps, out_fps, prefix: str):
    """pipeline.py:2128-2150."""
    _require_ffmpeg()
    fr_in = f"-framerate {in_fps}" if in_fps else ""
    fr_out = f"-r {out_fps}" if out_fps else ""
    if sorted(frames_dir.glob(f"{prefix}_*.jpg")):
        pattern = frames_dir / f"{prefix}_%04d.jpg"
    elif sorted(frames_dir.glob(f"{prefix}_*.png")):
        pattern = frames_dir / f"{prefix}_%04d.png"
    else:
        _log("No styled frames found (jpg/png).")
        sys.exit(1)
    sh(f'ffmpeg -y {fr_in} -i "{pattern}" {fr_out} -c:v libx264 -pix_fmt yuv420p "{output_video}"')


def parse_blend_weights(weights_str: Optional[str], num_models: int) -> List[float]:
    """pipeline.py:502-511."""
    if not weights_str:
        return [1.0 / num_models] * num_models
    weights = [float(w) for w in weights_str.split(",")]
    if len(weights) != num_models:
        raise ValueError(f"Expected {num_models} weights, got {len(weights)}")
    if abs(sum(weights) - 1.0) > 1e-6:
        raise ValueError(f"Weights must sum to 1.0, got {sum(weights):.6f}")
    return weights


def parse_lab_weights(weights_str: Optional[str]):
    """pipeline.py:514-521."""
    if not weights_str:
        return 0.5, 0.5
    wL, wab = [float(w) for w in weights_str.split(",")]
    if abs(wL + wab - 1.0) > 1e-6:
        raise ValueError(f"LAB weights must sum to 1.0, got {wL + wab:.6f}")
    return wL, wab


def lab_weights_rest(weights_str: Optional[str], num_models: int) -> List[float]:
    """pipeline.py:1843-1852: weights of models B.. for the LAB blend (the reference's length rule)."""
    w = parse_blend_weights(weights_str, max(num_models - 1, 1))
    if len(w) == 1:
        return [1.0]
    if len(w) in (2, 3):
        return w
    return [1.0 / max(num_models - 1, 1)] * max(num_models - 1, 1)


def _detect_transformer_type(checkpoint_path: str) -> str:
    """pipeline.py:72-79: NST_Train checkpoints have 'down1.' keys."""
    import torch
    state = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
    if isinstance(state, dict) and "state_dict" in state and isinstance(state["state_dict"], dict):
        state = state["state_dict"]
    return "nst" if any(k.startswith("down1.") for k in state.keys()) else "original"


def _load_checkpoint_compat(model, ckpt_path: str) -> None:
    """pipeline.py:554-569 (weights_only loads only: never unpickle arbitrary objects)."""
    import torch
    state = torch.load(ckpt_path, map_location="cpu", weights_only=True)
    if isinstance(state, dict) and "state_dict" in state and isinstance(state["state_dict"], dict):
        state = state["state_dict"]
    drop = ("running_mean", "running_var", "num_batches_tracked")
    state = {k: v for k, v in state.items() if not any(t in k for t in drop)}
    missing, unexpected = model.load_state_dict(state, strict=False)
    _log(f">> load_state_dict: missing={len(missing)} unexpected={len(unexpected)}")


_T7_LOADED: Dict[str, tuple] = {}  # resolved path -> (norm kind, parameters): prepare's check, reused by load_model


def load_torch7_or_exit(path: str, slot: str = "A"):
    """Read a Torch7 .t7 file and match it against the published fast-style architecture (host only).  A file that
    is missing, unreadable or not that architecture ends the run with code 2, as pipeline.py:594-596 does."""
    from ._lib import NstError
    from .torch7 import load_t7
    key = str(Path(path).resolve())
    if key not in _T7_LOADED:
        try:
            _T7_LOADED[key] = load_t7(key)
        except NstError as e:
            tag = "[torch7]" if slot == "A" else f"[torch7][{slot}]"
            _log(f"{tag}[ERROR] Could not load .t7 network from {path}: {e}")
            sys.exit(2)
    return _T7_LOADED[key]


def load_model(path: str, model_type: str, device, dtype: str, slot: str = "A", auto_nst: bool = True):
    """Model construction + load (pipeline.py:597-619; slots B..H always use the Johnson class for
    type transformer, :651-661 — kept)."""
    if model_type == "torch7":  # pipeline.py:583-596: the .t7 file on the engine instead of OpenCV DNN on the CPU
        from .torch7 import Torch7Net
        kind, params = load_torch7_or_exit(path, slot)
        model = Torch7Net(kind, params).to(device).eval()
        if dtype == "fp16m":  # as for ReCoNet: the split-precision head is built for the Johnson / NST nets
            _log("[backend] fp16m is built for the Johnson / NST nets; the Torch7 net runs fp32s (the same +-1 LSB bar)")
            dtype = "fp32s"
        model.compute_dtype = dtype
        _log(f"[backend] {slot}: type={model_type} path={path} device={device} arch=torch7_{kind} dtype={dtype}")
        return model, "torch7"
    if model_type == "reconet":
        from .model import ReCoNet
        model, arch = ReCoNet(), "reconet"
    else:
        arch = _detect_transformer_type(path) if auto_nst else "original"
        if arch == "nst":
            from .transformer_net_nst import TransformerNet
            _log(f"[model] Detected NST_Train architecture for {path}")
        else:
            from .transformer_net import TransformerNet
        model = TransformerNet()
    _load_checkpoint_compat(model, path)
    model = model.to(device).eval()
    if dtype == "fp16m" and arch == "reconet":  # the split-precision head is built for the 128-channel nets
        _log("[backend] fp16m is built for the Johnson / NST nets; ReCoNet runs fp32s (the same +-1 LSB bar)")
        dtype = "fp32s"
    model.compute_dtype = dtype
    _log(f"[backend] {slot}: type={model_type} path={path} device={device} arch={arch} dtype={dtype}")
    return model, arch


def load_stylizer(args, model_path, io_preset: str, dev):
    """Model A + optional B..H (RGB blend, pipeline.py:1872-1879), the region compositor and the blend weights
    -> (frame_loop.Stylizer, the io_preset in force)."""
    slots, slot_letters = [], []
    model_a, arch_a = load_model(str(model_path), args.model_type, dev, args.dtype, "A")
    if arch_a == "nst" and io_preset in ("auto", "raw_255", "imagenet_255"):  # pipeline.py:610-614
        _log(f"[model] Auto-switching io_preset from '{io_preset}' to 'raw_01' for NST_Train model")
        io_preset = "raw_01"
    # a Torch7 slot ignores its io_preset (pipeline.py:445-478) and hands on out01 = frame / 255 (:1443): toward the
    # fit, the blends, the regions and the temporal stage it is a raw_01 source (torch7.Torch7Engine)
    slots.append((model_a, "raw_01" if arch_a == "torch7" else io_preset))
    slot_letters.append(0)
    for li, s in enumerate(SLOTS, start=1):
        p = getattr(args, f"model_{s}", None)
        if not p:
            continue
        t = slot_model_type(args, s)
        ip = getattr(args, f"io_preset_{s}", None) or io_preset
        m, arch_s = load_model(p, t, dev, args.dtype, s.upper(), auto_nst=False)
        slots.append((m, "raw_01" if arch_s == "torch7" else ip))
        slot_letters.append(li)
    # pipeline.py:1519-1520: the standard path blends only when one of B, C, D is in use, and counts models as
    # 1 + B + C + D (slots E..H join the outputs list but the weights cover the first num_models of it)
    n_blend = 1 + sum(1 for s in SLOTS[:3] if getattr(args, f"model_{s}", None))
    regions = None
    if args.region_mode and (args.region_optimize or n_blend > 1):
        from .regions import RegionCompositor
        regions = RegionCompositor(args, dev)
        _log(f"[region] mode={args.region_mode} optimize={regions.optimized} seed={regions.seed}")
    lab = None
    if n_blend > 1 and getattr(args, "blend_models_lab", False):
        # LAB blend (pipeline.py:1841-1870): L from A, a/b from the weighted mix of the others
        lab_wl, lab_wab = parse_lab_weights(getattr(args, "blend_models_lab_weights", None))
        lab_rest = lab_weights_rest(args.blend_models_weights, n_blend)
        weights, lab = [lab_wl, lab_wab] + lab_rest, (lab_wl, lab_wab, lab_rest)
        _log(f"[blend] LAB blend: L={lab_wl},ab={lab_wab},rest={lab_rest}")
    else:
        weights = parse_blend_weights(args.blend_models_weights, n_blend) if n_blend > 1 else [1.0]
    return frame_loop.Stylizer(slots, slot_letters, n_blend, weights, lab, regions), io_preset


# ----------------------------------------------------------------------------- the frame loop
def style_frames(args, frames_dir: Optional[Path], model_path, output_prefix: str, image_ext_out: str, device_str: str,
                 threads: int, stride: int, max_frames: Optional[int], smooth_lightness: bool, smooth_alpha: float,
                 jpeg_quality: int, io_preset: str, smooth_chroma: bool = False, chroma_alpha: float = 0.85,
                 blend: float = 1.0, image_mode: bool = False, save_map: Optional[Dict[int, str]] = None,
                 rank: int = 0, world: int = 1):
    """Same signature/behaviour as pipeline.py:527-2122 (in-scope paths), GPU-batched: builds the parts of
    frame_loop.py and runs their stages."""
    import torch

    from .frames import agree_ok, plan_groups, rank0_share, run_pipeline, shard
    t_setup = time.perf_counter()
    from .postproc import LabSmoother

    # one GPU per rank (several ranks may share a device with --dist_backend gloo: tests)
    dev = torch.device("cuda", rank % torch.cuda.device_count() if world > 1 else torch.cuda.current_device())
    torch.cuda.set_device(dev)
    blend = float(max(0.0, min(1.0, blend)))
    stylizer, io_preset = load_stylizer(args, model_path, io_preset, dev)
    _log(f"[cfg] io_preset={io_preset} models={len(stylizer.slots)} weights={stylizer.weights} dtype={args.dtype} "
         f"gpus={world} batch={args.batch}")
    _log(f">> smoothing: {smooth_lightness}  alpha={smooth_alpha}  |  blend={blend}")
    src, names = frame_loop.list_frames(args, frames_dir, stride, max_frames)
    frame_loop.check_mask_dir(args, names)

    pool = ThreadPoolExecutor(max_workers=max(1, threads))
    prof = frame_loop.PipeProf()
    with prof("size_scan"):  # header reads (a PNG's EXIF lookup decodes it): on the pool
        sizes = list(pool.map(src.size, range(len(src))))
    # with --flow_ema rank 0 runs every frame's temporal stage (flow + fused EMA + LAB EMA + blend): a lighter share
    # of each group (frames.rank0_share).  Otherwise its ordered stage is the LAB EMA over 1-3 byte planes per
    # pixel (negligible), and every rank takes a full share.
    bsz = max(1, args.batch)
    flow_mode = bool(getattr(args, "flow_ema", False))
    r0 = rank0_share(world, bsz) if flow_mode else bsz
    caps = [r0] + [bsz] * (world - 1)
    groups = plan_groups(sizes, world, bsz, r0)
    my_shards = [shard(g, world, rank, caps) for g in groups]  # one per group, empty where this rank has no frames
    need_orig = blend < 1.0 or bool(args.mask or args.mask_dir) or (flow_mode and bool(getattr(args, "motion_blend", False)))
    lab = LabSmoother(dev, smooth_lightness, smooth_alpha, smooth_chroma, chroma_alpha)
    flow = None
    if flow_mode:
        from .temporal import FlowSmoother
        flow = FlowSmoother(True, float(args.flow_alpha), max(1, int(args.flow_downscale or 1)), args.flow_method)
    paths = frame_loop.OutputPaths(names, frames_dir, args.work_dir, output_prefix, image_ext_out, image_mode,
                                   save_map or {})
    sink = frame_loop.Sink(args, paths, jpeg_quality, pool, prof, dev)
    loop = frame_loop.FrameLoop(args, sizes, frame_loop.DecodeAhead(args, src, sizes, my_shards, pool, prof, dev),
                                stylizer, frame_loop.Masks(args, names, dev), sink, lab, flow, blend, need_orig,
                                total=len(src) if world == 1 else sum(len(s) for s in my_shards),
                                who=f" rank {rank}" if world > 1 else "", dev=dev)
    if loop.ordered:
        run_pipeline(groups, world, rank, loop.stylize_send, loop.root_post, loop.emit, loop.ret_spec, dev, caps)
    else:  # no ordered stage: every rank runs its frames start to finish, no exchange
        for mine in my_shards:
            err = None
            if mine:
                try:
                    _, full = loop.stylize_send(mine)
                    loop.emit(mine, None, full)
                except Exception as e:  # noqa: BLE001 -- re-raised below, after the other ranks have heard of it
                    err = e
            if world > 1:  # keep the ranks in step on errors, as run_pipeline does (RankFailed on the healthy ones)
                agree_ok(err is None, dev)
            if err is not None:
                raise err
    sink.drain()
    pool.shutdown()
    prof.report(rank)
    el = time.perf_counter() - loop.t_start
    written = [names[f] for f in sink.written]
    LAST_RUN_STATS.update(frames=len(src), seconds=el, setup_seconds=loop.t_start - t_setup, rank=rank, written=written)
    if os.environ.get("NST_PIPE_WRITTEN"):  # diagnostics: the frames this rank encoded and wrote (tests)
        import json
        with open(os.path.join(os.environ["NST_PIPE_WRITTEN"], f"rank{rank}.json"), "w") as fh:
            json.dump({"rank": rank, "world": world, "written": written, "loop_seconds": el,
                       "setup_seconds": loop.t_start - t_setup}, fh)
    if rank == 0:
        _log(f"Styled {len(src)}/{len(src)} frames in {el:.2f}s ({len(src) / max(el, 1e-9):.2f} frames/s)")


# ----------------------------------------------------------------------------- main
def _parse_canvas(s):
    if not s:
        return None
    wh = parse_wh(s)
    if not wh:
        _log(f"[canvas][ERROR] Expected WxH (e.g., 1920x1080), got: {s}")
        sys.exit(2)
    return wh


def prepare(args):
    """Mode decision + staging (pipeline.py:2430-2606). Returns (frames_dir, model_path, save_map, image_mode, video_mode)."""
    canvas_wh = _parse_canvas(getattr(args, "canvas", None))
    for k in ("input_video", "output_video", "input_image", "output_image", "input_dir", "output_dir"):
        v = getattr(args, k, None)
        if v is not None and str(v).strip() == "":
            setattr(args, k, None)
    if getattr(args, "pattern", None) in (None, ""):
        args.pattern = f"*.{args.image_ext}"
    image_single = bool(args.input_image) and bool(args.output_image)
    image_batch = bool(args.input_dir) and bool(args.output_dir)
    video = bool(args.input_video) and bool(args.output_video)
    synthetic = bool(args.synthetic)
    if (image_single or image_batch) and video:
        _log("Provide exactly one of: (input_video & output_video) OR (input_image & output_image) OR (input_dir & output_dir).")
        sys.exit(2)
    if not (image_single or image_batch or video or synthetic):
        _log("Specify (input_video & output_video) OR (input_image & output_image) OR (input_dir & output_dir).")
        sys.exit(2)
    if not args.model:
        _log("[error] --model is required")
        sys.exit(2)
    model_path = Path(args.model).resolve()
    if model_path.suffix.lower() == ".t7":
        args.model_type = "torch7"
    if args.io_preset == "auto":
        args.io_preset = IO_PRESETS_AUTO.get(args.model_type, "imagenet_01")
        _log(f"[auto] io_preset resolved to '{args.io_preset}' for backend '{args.model_type}'")
    reject_out_of_scope(args)
    # Torch7 slots: read and match the files now, before anything is staged (exit 2 on a bad one, :594-596, :648-650)
    if args.model_type == "torch7":
        load_torch7_or_exit(str(model_path), "A")
    for s in SLOTS:
        if getattr(args, f"model_{s}", None) and slot_model_type(args, s) == "torch7":
            load_torch7_or_exit(str(getattr(args, f"model_{s}")), s.upper())
    save_map: Dict[int, str] = {}
    base_work = Path(args.work_dir).resolve()
    if synthetic:
        return None, model_path, save_map, False, False
    work_dir = base_work / f"job_{uuid.uuid4().hex[:8]}" if (image_single or image_batch) else base_work
    frames_dir = work_dir / "frames"
    if frames_dir.exists() and video:
        shutil.rmtree(frames_dir, ignore_errors=True)
    frames_dir.mkdir(parents=True, exist_ok=True)
    if video:
        in_v = Path(args.input_video).resolve()
        if args.pre_fps:
            tmp = work_dir / f"prefps_{args.pre_fps}.mp4"
            _require_ffmpeg()
            sh(f'ffmpeg -y -i "{in_v}" -vf fps={args.pre_fps} -c:v libx264 -pix_fmt yuv420p "{tmp}"')
            in_v = tmp
        extract_frames(in_v, frames_dir, args.fps if not args.pre_fps else None, args.scale, args.image_ext,
                       args.jpeg_quality, canvas_wh)
    elif image_single:
        src = Path(args.input_image).resolve()
        ext = src.suffix.lower() if src.suffix.lower() in (".png", ".jpg", ".jpeg") else ".png"
        dst = frames_dir / f"frame_0001{ext}"
        pil = _get_image_with_exif_pil(str(src))
        if ext in (".jpg", ".jpeg"):
            pil.save(dst, format="JPEG", quality=max(1, min(95, int(args.jpeg_quality))))
        else:
            pil.save(dst)
        save_map[1] = str(Path(args.output_image).resolve())
    else:
        in_files = sorted(glob.glob(os.path.join(args.input_dir, args.pattern)))
        if not in_files:
            _log(f"No files matched: {args.input_dir}/{args.pattern}")
            sys.exit(2)
        Path(args.output_dir).mkdir(parents=True, exist_ok=True)

        # the reference's per-file staging copy (pipeline.py:2560-2590: EXIF-upright RGB re-saved as
        # frames/frame_{i:04d}{ext}, JPEG at --jpeg_quality) happens in memory when the frame is loaded
        # (FrameSource._open_rgb): a PNG copy decodes to that RGB image itself, a JPEG copy is re-encoded and
        # decoded from memory -- the same pixels without writing the staged files (--keep_staged writes them too)
        q = max(1, min(95, int(args.jpeg_quality)))
        args._staged_sources = [(Path(f).resolve(), q if Path(f).suffix.lower() in (".jpg", ".jpeg") else None)
                                for f in in_files]
        if getattr(args, "keep_staged", False):
            def stage(i_f):
                i, f = i_f
                src = Path(f).resolve()
                ext = src.suffix.lower()
                pil = _get_image_with_exif_pil(str(src))
                dst = frames_dir / f"frame_{i:04d}{ext}"
                if ext in (".jpg", ".jpeg"):
                    pil.save(dst, format="JPEG", quality=q)
                else:
                    pil.save(dst)
            with ThreadPoolExecutor(max_workers=max(1, int(getattr(args, "threads", 1) or 1))) as ex:
                list(ex.map(stage, enumerate(in_files, start=1)))
        for i, f in enumerate(in_files, start=1):
            src = Path(f).resolve()
            ext = src.suffix.lower()
            base = src.stem
            out_ext = ext if args.keep_ext else (".jpg" if args.image_ext.lower() == "jpg" else ".png")
            m = re.match(r"^frame_(\d+)$", base)
            out_stem = f"{args.output_prefix}_{m.group(1)}" if m else f"{base}{args.output_suffix or ''}"
            save_map[i] = str((Path(args.output_dir) / f"{out_stem}{out_ext}").resolve())
    return frames_dir, model_path, save_map, (image_single or image_batch), video


def _worker(rank: int, world: int, argv: List[str], port: int, prep, staged=None):
    import torch
    import torch.distributed as dist
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    args = build_parser().parse_args(argv)
    if staged is not None:  # --input_dir sources staged in memory by the parent's prepare()
        args._staged_sources = staged
    dev = torch.device("cuda", rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    if args.dist_backend == "nccl":  # RCCL over xGMI, one GPU per rank
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                                device_id=dev, timeout=timedelta(seconds=args.dist_timeout))
    else:  # gloo: frames travel through host memory (ranks may share a GPU)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                                timeout=timedelta(seconds=args.dist_timeout))
    try:
        frames_dir, model_path, save_map, image_mode, _ = prep
        _run_style(args, frames_dir, model_path, save_map, image_mode, rank, world)
    finally:
        dist.destroy_process_group()


def _run_style(args, frames_dir, model_path, save_map, image_mode, rank=0, world=1):
    return style_frames(args, frames_dir, model_path, output_prefix="styled_frame", image_ext_out=args.image_ext,
                        device_str=args.device, threads=args.threads, stride=args.stride, max_frames=args.max_frames,
                        smooth_lightness=args.smooth_lightness, smooth_alpha=args.smooth_alpha,
                        jpeg_quality=args.jpeg_quality, io_preset=args.io_preset, smooth_chroma=args.smooth_chroma,
                        chroma_alpha=args.chroma_alpha, blend=args.blend, image_mode=image_mode, save_map=save_map,
                        rank=rank, world=world)


def main(argv: Optional[List[str]] = None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    args = build_parser().parse_args(argv)
    prep = prepare(args)
    frames_dir, model_path, save_map, image_mode, video = prep
    # re-parse inside workers with the resolved preset/model type
    resolved = argv + ["--io_preset", args.io_preset, "--model_type", args.model_type]
    if args.gpus > 1:
        import socket

        import torch.multiprocessing as mp
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        mp.start_processes(_worker, args=(args.gpus, resolved, port, prep, getattr(args, "_staged_sources", None)), nprocs=args.gpus, start_method="spawn")
    else:
        _run_style(args, frames_dir, model_path, save_map, image_mode)
    if video:
        in_fps = int(args.pre_fps) if args.pre_fps else (int(args.fps) if args.fps else None)
        out_fps = int(args.fps) if (args.pre_fps and args.fps) else None
        assemble_video(frames_dir, Path(args.output_video).resolve(), in_fps, out_fps, prefix="styled_frame")
        _log(f"\n Done. Styled video at: {Path(args.output_video).resolve()}")
    elif image_mode:
        written = sum(1 for v in save_map.values() if Path(v).exists())
        _log(f"Wrote {written}/{len(save_map)} image(s)")
    if args.clean_frames and frames_dir is not None:
        for pat in ("frame_*.png", "frame_*.jpg", "styled_frame_*.png", "styled_frame_*.jpg"):
            for p in frames_dir.glob(pat):
                p.unlink(missing_ok=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
