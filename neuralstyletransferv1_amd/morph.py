"""Optical-flow morph between stills on the MI355X engine: the reference's `optical_flow_morph`
(scripts/optical_flow_slideshow.py:17-70, scripts/morph_v2.py:365-468 and the copies in morph_faces.py,
generate_morph_samples.py and the optical_flow_* batch scripts) and a CLI that turns a list of stills into the
frames of a morphing slideshow.

Per transition img1 -> img2 (RGB uint8 device tensors of one size):
  gray = cv2.cvtColor(img, COLOR_BGR2GRAY)                          nst_gray_cv_u8
  gray = cv2.GaussianBlur(gray, (5, 5), 1.0)          (preset v2)   nst_gauss_u8
  fwd, bwd = cv2.calcOpticalFlowFarneback(g1, g2 | g2, g1, ..., OPTFLOW_FARNEBACK_GAUSSIAN)
                                                                    nst_flow_farneback_ex, n = 2 in the same launches
  blur 15x15 sigma 3 + radial minimum flow            (preset v2)   nst_morph_flow_post
  k frames: two cv2.remap(INTER_LINEAR, BORDER_REFLECT) + cv2.addWeighted
                                                                    nst_morph_frames, all frames of a launch at once

Presets (the reference's two parameter sets):
  slideshow  Farneback 0.5 / 5 / 15 / 3 / 7 / 1.5, no pre-blur, no post-processing, t = alpha = i / (k - 1)
  v2         pre-blur, Farneback 0.5 / 6 / 21 / 5 / 7 / 1.5, flow post-processing, t = ease(i / (k - 1)) with
             ease in linear | smooth (cubic in/out) | smoother (smootherstep), alpha = smoothstep(i / (k - 1))
k = 1 gives t = 0 in both.  The schedules are computed in double and rounded once to the fp32 the kernel multiplies
by (t, 1 - t, 1 - alpha, alpha).

Stills are decoded with Pillow and fitted by cover + centre crop with morph_v2.py:704-712's sizes (int(w * scale),
(new - target) // 2); the resize is the engine's Pillow-exact LANCZOS (Image.resize(LANCZOS)) and REPLACES the
reference's cv2.INTER_LANCZOS4 (an 8-tap kernel without Pillow's support scaling): fitted stills differ from the
reference's.  cv2 is not installed in this environment, so the grey, blur, Farneback, remap and addWeighted
restatements are parity unpinned; tests/morph_ref.py is their numpy yardstick.

With --pan_zoom > 1 the CLI is create_morph_video's Ken Burns path (morph_v2.py:839-948): the stills load at pan
size (camera.load_for_pan), the morph runs at that size, and every output frame -- held frames included -- goes
through the camera stage of camera.py on the device (zoom pulse, zoom-in phase, sub-pixel pan, hue rotation) by its
global index g, progress = g / max(1, total - 1); temporal_smooth_frames then runs over the whole sequence, streamed
with kernel_size // 2 frames of halo between batches.  With --hold_frames 0 the frame count and the progress are the
reference's.  Without --pan_zoom nothing changes, and the camera flags are refused (the reference silently ignores
them).

Out of scope (not built): morph_v2's DeepLab and Magenta orchestration, its crossfade fallback after a failed morph,
cv2's video writer, and morph_faces.py's face detection.
"""
from __future__ import annotations

import argparse
import ctypes
import sys
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, stills
from ._lib import NstError, check, lib
from .stills import FrameWriter, ease_in_out_cubic, smoothstep

# pyr_scale, levels, winsize, iterations, poly_n, poly_sigma
PRESETS = {
    "slideshow": dict(farneback=(0.5, 5, 15, 3, 7, 1.5), pre_blur=False, post=False),
    "v2": dict(farneback=(0.5, 6, 21, 5, 7, 1.5), pre_blur=True, post=True),
}
EASINGS = ("linear", "smooth", "smoother")
IMAGE_PATTERNS = ("*.jpg", "*.jpeg", "*.png")
PAN_DIRECTIONS = ("horizontal", "vertical", "diagonal", "diagonal_reverse")


def smootherstep(t: float) -> float:
    return t * t * t * (t * (6 * t - 15) + 10)


_EASE = {"linear": lambda t: t, "smooth": ease_in_out_cubic, "smoother": smootherstep}


def schedule(k: int, preset: str = "v2", easing: str = "smooth") -> Tuple[np.ndarray, np.ndarray]:
    """(t, alpha) of the k frames of a transition, float64."""
    if preset not in PRESETS:
        raise ValueError(f"preset must be one of {sorted(PRESETS)}, got {preset!r}")
    if easing not in _EASE:
        raise ValueError(f"easing must be one of {EASINGS}, got {easing!r}")
    if k < 1:
        raise ValueError(f"a transition needs at least one frame, got {k}")
    lin = [i / (k - 1) if k > 1 else 0.0 for i in range(k)]
    if preset == "slideshow":
        return np.array(lin, np.float64), np.array(lin, np.float64)
    return np.array([_EASE[easing](x) for x in lin], np.float64), np.array([smoothstep(x) for x in lin], np.float64)


def kernel_schedule(t: np.ndarray, alpha: np.ndarray):
    """The four fp32 rows nst_morph_frames takes: t, 1 - t, 1 - alpha, alpha (each computed in double, rounded once)."""
    return (t.astype(np.float32), (1.0 - t).astype(np.float32), (1.0 - alpha).astype(np.float32),
            alpha.astype(np.float32))


def _u8(x: torch.Tensor, what: str, dims: int) -> torch.Tensor:
    _lib.require_gpu_tensor(x, what)
    if x.dtype != torch.uint8 or x.dim() != dims:
        raise NstError(f"{what}: expected a uint8 tensor of {dims} dimensions, got {x.dtype} {tuple(x.shape)}")
    return x.contiguous()


def gray_cv_u8(frames_u8: torch.Tensor) -> torch.Tensor:
    """[n,h,w,3] uint8 RGB -> [n,h,w] uint8, cv2's 8-bit COLOR_BGR2GRAY weights."""
    x = _u8(frames_u8, "gray_cv_u8 frames", 4)
    n, h, w, _ = x.shape
    out = torch.empty((n, h, w), dtype=torch.uint8, device=x.device)
    check(lib().nst_gray_cv_u8(x.data_ptr(), n, h, w, out.data_ptr(), _lib.stream_ptr(x.device)), "nst_gray_cv_u8")
    return out


def gauss_u8(gray: torch.Tensor) -> torch.Tensor:
    """[n,h,w] uint8 -> cv2.GaussianBlur(g, (5, 5), 1.0) restated in fp32."""
    x = _u8(gray, "gauss_u8 images", 3)
    n, h, w = x.shape
    out = torch.empty_like(x)
    check(lib().nst_gauss_u8(x.data_ptr(), n, h, w, out.data_ptr(), _lib.stream_ptr(x.device)), "nst_gauss_u8")
    return out


def farneback_ex(prev: torch.Tensor, nxt: torch.Tensor, params, flags: int = 0) -> torch.Tensor:
    """n pairs [n,h,w] uint8 x 2 -> flows [n,h,w,2] float32 in the same launches; flags 0 or NST_FLOW_GAUSSIAN."""
    p, q = _u8(prev, "farneback_ex prev", 3), _u8(nxt, "farneback_ex next", 3)
    if p.shape != q.shape:
        raise NstError(f"farneback_ex: shapes differ, {tuple(p.shape)} and {tuple(q.shape)}")
    n, h, w = p.shape
    dev = p.device
    sz = ctypes.c_size_t()
    check(lib().nst_flow_scratch_floats_ex(n, h, w, ctypes.byref(sz)), "nst_flow_scratch_floats_ex")
    sc = torch.empty((sz.value,), dtype=torch.float32, device=dev)
    flow = torch.empty((n, h, w, 2), dtype=torch.float32, device=dev)
    ps, lv, ws, it, pn, sg = params
    check(lib().nst_flow_farneback_ex(p.data_ptr(), q.data_ptr(), n, h, w, float(ps), int(lv), int(ws), int(it), int(pn),
                                      float(sg), int(flags), flow.data_ptr(), sc.data_ptr(), sc.numel(),
                                      _lib.stream_ptr(dev)), "nst_flow_farneback_ex")
    sc.record_stream(torch.cuda.current_stream(dev))
    return flow


def flow_post(flow: torch.Tensor, signs: Sequence[float]) -> torch.Tensor:
    """morph_v2.py:405-432 on flows [n,h,w,2] (a copy is returned): blur, then the radial term with signs[n]."""
    _lib.require_gpu_tensor(flow, "flow_post flow")
    if flow.dtype != torch.float32 or flow.dim() != 4 or flow.shape[3] != 2 or len(signs) != flow.shape[0]:
        raise NstError(f"flow_post: expected float32 [n,h,w,2] and n signs, got {flow.dtype} {tuple(flow.shape)}")
    out = flow.contiguous().clone()
    n, h, w, _ = out.shape
    scratch = torch.empty_like(out)
    sg = (ctypes.c_float * n)(*[float(s) for s in signs])
    check(lib().nst_morph_flow_post(out.data_ptr(), n, h, w, sg, scratch.data_ptr(), _lib.stream_ptr(out.device)),
          "nst_morph_flow_post")
    scratch.record_stream(torch.cuda.current_stream(out.device))
    return out


def morph_frames(img1: torch.Tensor, img2: torch.Tensor, fwd: torch.Tensor, bwd: torch.Tensor, t: np.ndarray,
                 alpha: np.ndarray, batch: Optional[int] = None) -> torch.Tensor:
    """The frames of a transition, uint8 [k,h,w,3]: `batch` frames per nst_morph_frames launch (default: as many as
    one launch takes)."""
    a, b = _u8(img1, "morph_frames img1", 3), _u8(img2, "morph_frames img2", 3)
    h, w, c = a.shape
    if c != 3 or b.shape != a.shape:
        raise NstError(f"morph_frames: images must both be [h,w,3], got {tuple(a.shape)} and {tuple(b.shape)}")
    for f in (fwd, bwd):
        _lib.require_gpu_tensor(f, "morph_frames flow")
        if f.dtype != torch.float32 or tuple(f.shape) != (h, w, 2):
            raise NstError(f"morph_frames: flows must be float32 [{h},{w},2], got {f.dtype} {tuple(f.shape)}")
    fwd, bwd = fwd.contiguous(), bwd.contiguous()
    k = len(t)
    step = _lib.NST_MORPH_MAX_FRAMES if not batch else max(1, min(int(batch), _lib.NST_MORPH_MAX_FRAMES))
    rows = kernel_schedule(np.asarray(t, np.float64), np.asarray(alpha, np.float64))
    out = torch.empty((k, h, w, 3), dtype=torch.uint8, device=a.device)
    pf = ctypes.POINTER(ctypes.c_float)
    for s in range(0, k, step):
        e = min(k, s + step)
        r = [np.ascontiguousarray(x[s:e]) for x in rows]
        check(lib().nst_morph_frames(a.data_ptr(), b.data_ptr(), fwd.data_ptr(), bwd.data_ptr(), h, w, e - s,
                                     *[x.ctypes.data_as(pf) for x in r], out[s:e].data_ptr(),
                                     _lib.stream_ptr(a.device)), "nst_morph_frames")
    return out


def morph_flows(img1_u8: torch.Tensor, img2_u8: torch.Tensor, preset: str = "v2") -> Tuple[torch.Tensor, torch.Tensor]:
    """(forward, backward) flows [h,w,2] of a transition, post-processed as the preset says."""
    if preset not in PRESETS:
        raise ValueError(f"preset must be one of {sorted(PRESETS)}, got {preset!r}")
    p = PRESETS[preset]
    a, b = _u8(img1_u8, "optical_flow_morph img1", 3), _u8(img2_u8, "optical_flow_morph img2", 3)
    if a.shape != b.shape or a.shape[2] != 3:
        raise NstError(f"optical_flow_morph: images must both be [h,w,3], got {tuple(a.shape)} and {tuple(b.shape)}")
    g = gray_cv_u8(torch.stack([a, b]))
    if p["pre_blur"]:
        g = gauss_u8(g)
    flows = farneback_ex(g, g.flip(0), p["farneback"], _lib.NST_FLOW_GAUSSIAN)  # (g1, g2) and (g2, g1)
    if p["post"]:
        flows = flow_post(flows, (1.0, -1.0))
    return flows[0], flows[1]


def optical_flow_morph(img1_u8: torch.Tensor, img2_u8: torch.Tensor, num_interp_frames: int = 72, preset: str = "v2",
                       easing: str = "smooth", batch: Optional[int] = None) -> torch.Tensor:
    """RGB uint8 [h,w,3] device tensors -> the transition's frames, uint8 [k,h,w,3]."""
    t, alpha = schedule(int(num_interp_frames), preset, easing)
    fwd, bwd = morph_flows(img1_u8, img2_u8, preset)
    return morph_frames(img1_u8, img2_u8, fwd, bwd, t, alpha, batch)


# ---- CLI ----
def cover_geometry(w: int, h: int, tw: int, th: int) -> Tuple[int, int, int, int]:
    """morph_v2.py:704-712: (new_w, new_h, start_x, start_y) of cover + centre crop.  int(w * scale) can fall one
    short of the target through the float product; the size is then the target (the reference would crop short)."""
    scale = max(tw / w, th / h)
    nw, nh = max(int(w * scale), tw), max(int(h * scale), th)
    return nw, nh, (nw - tw) // 2, (nh - th) // 2


def list_images(images_dir: Optional[str], images: Optional[Sequence[str]]) -> List[Path]:
    """--images in the order given; --images_dir: every *.jpg, *.jpeg, *.png, sorted by path (the slideshow's rule)."""
    if images:
        return [Path(p) for p in images]
    files: List[Path] = []
    for pat in IMAGE_PATTERNS:
        files.extend(Path(images_dir).glob(pat))
    return sorted(files, key=str)


def total_frames(n_images: int, k: int, hold_frames: int, hold_end: int) -> int:
    return n_images * hold_frames + (n_images - 1) * k + hold_end


def parse_size(s: str) -> Tuple[int, int]:
    try:
        w, h = (int(v) for v in s.lower().split("x"))
    except ValueError:
        raise argparse.ArgumentTypeError(f"size must be WxH, got {s!r}")
    if w < 2 or h < 2:
        raise argparse.ArgumentTypeError(f"size must be at least 2x2, got {s!r}")
    return w, h


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m neuralstyletransferv1_amd.morph",
                                 description="Optical-flow morph slideshow between stills on the GPU")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--images_dir", type=str, help="directory of stills (*.jpg, *.jpeg, *.png, sorted)")
    src.add_argument("--images", type=str, nargs="+", help="stills in slideshow order")
    ap.add_argument("--size", type=parse_size, default=(1920, 1080), help="output WxH")
    ap.add_argument("--fps", type=float, default=24.0)
    ap.add_argument("--morph_seconds", type=float, default=2.0, help="frames per transition = int(fps * seconds)")
    ap.add_argument("--preset", choices=sorted(PRESETS), default="v2")
    ap.add_argument("--easing", choices=EASINGS, default="smooth", help="warp timing of preset v2")
    ap.add_argument("--hold_frames", type=int, default=0, help="frames each still is shown before its transition")
    ap.add_argument("--hold_end", type=int, default=24, help="extra frames of the last still")
    stills.add_output_flags(ap, "morph_frame")
    ap.add_argument("--output_video", type=str, default=None, help="also assemble the frames with ffmpeg")
    ap.add_argument("--batch", type=int, default=24, help="frames per nst_morph_frames launch (and per write)")
    ap.add_argument("--device", type=str, default="cuda:0")
    cam = ap.add_argument_group("camera (morph_v2's Ken Burns path; all of it needs --pan_zoom > 1)")
    cam.add_argument("--pan_zoom", type=float, default=None, help="morph at pan_zoom x the output size and pan across")
    cam.add_argument("--pan_direction", choices=PAN_DIRECTIONS, default=None, help="default horizontal")
    cam.add_argument("--zoom_in_pct", type=float, default=None, help="share of the video spent zooming in (default 0.25)")
    cam.add_argument("--zoom_pulse", type=float, default=0.0, help="amplitude of the zoom pulse (0 = off)")
    cam.add_argument("--zoom_pulse_freq", type=float, default=None, help="pulse cycles per video (default 2.0)")
    cam.add_argument("--hue_rotate", type=float, default=0.0, help="total hue rotation in degrees over the video")
    cam.add_argument("--temporal_smooth", type=int, default=0, help="temporal smoothing kernel in frames (0 = off)")
    cam.add_argument("--zoom", type=float, default=None, help="static centre zoom of every still before the pan scale")
    return ap


def camera_argument_error(args) -> Optional[str]:
    """The message of a bad combination of camera flags, or None.  No device is touched."""
    given = [name for name, on in (
        ("--pan_direction", args.pan_direction is not None), ("--zoom_in_pct", args.zoom_in_pct is not None),
        ("--zoom_pulse", args.zoom_pulse != 0), ("--zoom_pulse_freq", args.zoom_pulse_freq is not None),
        ("--hue_rotate", args.hue_rotate != 0), ("--temporal_smooth", args.temporal_smooth != 0),
        ("--zoom", args.zoom is not None)) if on]
    if args.pan_zoom is None:
        return f"{', '.join(given)} need(s) --pan_zoom > 1 (the camera stage runs only then)" if given else None
    if not args.pan_zoom > 1.0:
        return f"--pan_zoom must be greater than 1, got {args.pan_zoom}"
    if args.zoom_in_pct is not None and not 0.0 <= args.zoom_in_pct <= 1.0:
        return f"--zoom_in_pct must lie in [0, 1], got {args.zoom_in_pct}"
    if args.zoom_pulse < 0 or not args.zoom_pulse <= 1.0:
        return f"--zoom_pulse must lie in [0, 1], got {args.zoom_pulse}"
    if not 0 <= args.temporal_smooth <= _lib.NST_CAMERA_MAX_SMOOTH:
        return f"--temporal_smooth must lie in 0..{_lib.NST_CAMERA_MAX_SMOOTH}, got {args.temporal_smooth}"
    if args.zoom is not None and not args.zoom >= 1.0:
        return f"--zoom must be at least 1, got {args.zoom}"
    return None


def pan_size(files: Sequence[Path], tw: int, th: int, pan_zoom: float, zoom: float) -> Tuple[Optional[Tuple[int, int]], Optional[str]]:
    """((w, h) the stills share at pan size, None) or (None, the error): read from the image headers, no device."""
    from PIL import Image

    from .camera import pan_geometry
    size = None
    for f in files:
        with Image.open(f) as im:
            w, h = im.size
        nw, nh = pan_geometry(w, h, tw, th, pan_zoom, zoom)[4:]
        if nw < tw or nh < th:
            return None, f"{f}: its pan size {nw}x{nh} is smaller than the output {tw}x{th}"
        if size is None:
            size = (nw, nh)
        elif (nw, nh) != size:
            return None, f"{f}: its pan size {nw}x{nh} differs from {files[0]}'s {size[0]}x{size[1]}"
    return size, None


def load_fitted(path: Path, tw: int, th: int, device: torch.device) -> torch.Tensor:
    """Pillow decode -> RGB -> cover (GPU LANCZOS) -> centre crop: uint8 [th,tw,3] on the device."""
    from PIL import Image

    from .deeplab import Resampler
    with Image.open(path) as im:
        rgb = np.array(im.convert("RGB"), dtype=np.uint8)
    h, w = rgb.shape[:2]
    nw, nh, sx, sy = cover_geometry(w, h, tw, th)
    x = torch.from_numpy(rgb).to(device)[None]
    if (nw, nh) != (w, h):
        x = Resampler("lanczos", h, w, nh, nw, device)(x)
    return x[0, sy:sy + th, sx:sx + tw].contiguous()


def _hold(wr: FrameWriter, img: torch.Tensor, n: int, step: int) -> None:
    for s in range(0, n, step):
        wr.write(img[None].repeat(min(step, n - s), 1, 1, 1))


def _main_camera(args, files: Sequence[Path], k: int, size: Tuple[int, int]) -> int:
    """The --pan_zoom path: every output frame through the camera stage by its global index."""
    from . import camera as CAM
    device = torch.device(args.device)
    tw, th = args.size
    zoom = args.zoom if args.zoom is not None else 1.0
    wr = stills.open_writer(args)
    total = total_frames(len(files), k, args.hold_frames, args.hold_end)
    plan = CAM.frame_plan(total, size, (tw, th), args.pan_zoom, args.pan_direction or "horizontal",
                          0.25 if args.zoom_in_pct is None else args.zoom_in_pct, args.zoom_pulse,
                          2.0 if args.zoom_pulse_freq is None else args.zoom_pulse_freq, args.hue_rotate)
    smooth = CAM.SmoothStream(total, args.temporal_smooth)
    t, alpha = schedule(k, args.preset, args.easing)
    step = max(1, min(args.batch, _lib.NST_MORPH_MAX_FRAMES))
    g = 0

    def emit(frames: torch.Tensor) -> None:
        nonlocal g
        n = frames.shape[0]
        done = smooth.push(CAM.camera_frames(frames, plan[g:g + n], (tw, th)))
        g += n
        if done is not None:
            wr.write(done)

    def hold(img: torch.Tensor, n: int) -> None:
        for s in range(0, n, step):
            emit(img[None].repeat(min(step, n - s), 1, 1, 1))

    cur = CAM.load_for_pan(files[0], tw, th, args.pan_zoom, zoom, device)
    for idx in range(len(files)):
        hold(cur, args.hold_frames)
        if idx + 1 < len(files):
            nxt = CAM.load_for_pan(files[idx + 1], tw, th, args.pan_zoom, zoom, device)
            fwd, bwd = morph_flows(cur, nxt, args.preset)
            for s in range(0, k, step):
                emit(morph_frames(cur, nxt, fwd, bwd, t[s:s + step], alpha[s:s + step]))
            cur = nxt
        print(f"[morph] {idx + 1}/{len(files)} {files[idx].name}: {g} frames")
    hold(cur, args.hold_end)
    assert g == total and wr.count == total
    stills.close_run("morph", wr, args.fps, args.output_video)
    return 0


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = build_parser().parse_args(argv)
    files = list_images(args.images_dir, args.images)
    if len(files) < 2:
        print(f"[morph] need at least 2 images, got {len(files)}", file=sys.stderr)
        return 2
    k = int(args.fps * args.morph_seconds)
    if k < 1 or args.hold_frames < 0 or args.hold_end < 0 or args.batch < 1:
        print("[morph] need int(fps * morph_seconds) >= 1, hold counts >= 0 and --batch >= 1", file=sys.stderr)
        return 2
    err = camera_argument_error(args)
    if err is None and args.pan_zoom is not None:
        size, err = pan_size(files, args.size[0], args.size[1], args.pan_zoom, args.zoom if args.zoom is not None else 1.0)
    if err is not None:
        print(f"[morph] {err}", file=sys.stderr)
        return 2
    if args.pan_zoom is not None:
        return _main_camera(args, files, k, size)
    device = torch.device(args.device)
    tw, th = args.size
    wr = stills.open_writer(args)
    t, alpha = schedule(k, args.preset, args.easing)
    step = max(1, min(args.batch, _lib.NST_MORPH_MAX_FRAMES))
    cur = load_fitted(files[0], tw, th, device)
    for idx in range(len(files)):
        _hold(wr, cur, args.hold_frames, step)
        if idx + 1 < len(files):
            nxt = load_fitted(files[idx + 1], tw, th, device)
            fwd, bwd = morph_flows(cur, nxt, args.preset)
            for s in range(0, k, step):
                wr.write(morph_frames(cur, nxt, fwd, bwd, t[s:s + step], alpha[s:s + step]))
            cur = nxt
        print(f"[morph] {idx + 1}/{len(files)} {files[idx].name}: {wr.count} frames")
    _hold(wr, cur, args.hold_end, step)
    assert wr.count == total_frames(len(files), k, args.hold_frames, args.hold_end)
    stills.close_run("morph", wr, args.fps, args.output_video)
    return 0


if __name__ == "__main__":
    sys.exit(main())
