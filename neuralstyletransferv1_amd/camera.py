"""The camera stage of the morph slideshow on the MI355X engine: what the reference's create_morph_video
(scripts/morph_v2.py:624-999) does to every morph frame when --pan_zoom is given, between optical_flow_morph and the
video writer.

Per output frame g of `total` (progress = g / max(1, total - 1)):
  zoom pulse   cv2.resize(frame, int(size * pulse), INTER_LINEAR) + centre crop          nst_camera_pulse_u8
  zoom phase   getRectSubPix(frame, crop, centre) + resize(target, INTER_LANCZOS4)       nst_camera_rect_subpix_u8,
               (progress < zoom_in_pct)                                                  nst_camera_lanczos_u8
  pan phase    getRectSubPix(frame, target, (x + tw / 2, y + th / 2))                    nst_camera_rect_subpix_u8
  hue          apply_hue_shift(frame, progress * hue_rotate)                             nst_camera_hue_u8
and over the whole sequence temporal_smooth_frames (nst_camera_smooth_u8).  The CLI runs the first four as one call,
nst_camera_frames_u8 (camera_frames): two launches per batch of morph frames, each frame its own steps.

frame_plan() is pure Python and needs no GPU: extract_pan_frame, calculate_zoom_pulse and progress * hue_rotate in
double with the script's own int() truncations and clamps, one CameraFrame per global frame index.

cv2 is not installed in this environment, so parity with OpenCV is unpinned; tests/camera_ref.py
is the numpy yardstick, and the kernels equal it byte for byte.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import NstCameraFrame, NstError, check, lib
from .stills import ease_in_out_cubic

PAN_DIRECTIONS = ("horizontal", "vertical", "diagonal", "diagonal_reverse")
MAX_FRAMES = _lib.NST_CAMERA_MAX_FRAMES
f32 = np.float32


# ---- the plan (no GPU) ----
@dataclass(frozen=True)
class CameraFrame:
    progress: float
    pulse_w: int      # the pulse's resized size; the frame's own size: no pulse
    pulse_h: int
    zoom: bool        # zoom phase (patch -> Lanczos to the target) or pan phase (patch = target)
    patch_w: int
    patch_h: int
    cx: float         # getRectSubPix centre, double (the kernel takes it as float32, as cv2 does)
    cy: float
    hue_shift: float  # degrees; |shift| < 0.1 leaves the frame alone


def calculate_zoom_pulse(progress: float, amplitude: float, frequency: float) -> float:
    """morph_v2.py:348-362 (np.sin, as the script)."""
    return 1.0 + abs(np.sin(progress * frequency * 2 * np.pi)) * amplitude


def extract_pan_geometry(progress: float, w: int, h: int, tw: int, th: int, pan_zoom: float, direction: str,
                         zoom_in_pct: float) -> Tuple[bool, int, int, float, float]:
    """extract_pan_frame (morph_v2.py:746-831) without the pixels: (zoom phase, patch_w, patch_h, cx, cy)."""
    if progress < zoom_in_pct and zoom_in_pct > 0:
        eased = ease_in_out_cubic(progress / zoom_in_pct)
        start_w, start_h = min(w, int(tw * pan_zoom)), min(h, int(th * pan_zoom))
        crop_w = max(tw, int(start_w + (tw - start_w) * eased))
        crop_h = max(th, int(start_h + (th - start_h) * eased))
        return True, crop_w, crop_h, w / 2.0, h / 2.0
    pan_progress = (progress - zoom_in_pct) / (1.0 - zoom_in_pct) if zoom_in_pct < 1.0 else 0.0
    max_x, max_y = w - tw, h - th
    eased = ease_in_out_cubic(pan_progress)
    if direction == "vertical":
        x, y = max_x / 2.0, (max_y / 2.0) + eased * (max_y / 2.0)
    elif direction == "diagonal":
        x, y = (max_x / 2.0) + eased * (max_x / 2.0), (max_y / 2.0) + eased * (max_y / 2.0)
    elif direction == "diagonal_reverse":
        x, y = (max_x / 2.0) - eased * (max_x / 2.0), (max_y / 2.0) + eased * (max_y / 2.0)
    else:  # horizontal, and the script's fallback
        x, y = (max_x / 2.0) + eased * (max_x / 2.0), max_y / 2.0
    x = max(0.0, min(x, float(max_x)))
    y = max(0.0, min(y, float(max_y)))
    return False, tw, th, x + tw / 2.0, y + th / 2.0


def frame_plan(total: int, size: Tuple[int, int], target: Tuple[int, int], pan_zoom: float,
               pan_direction: str = "horizontal", zoom_in_pct: float = 0.25, zoom_pulse: float = 0.0,
               zoom_pulse_freq: float = 2.0, hue_rotate: float = 0.0) -> List[CameraFrame]:
    """One CameraFrame per global frame index; size = the morph frames' (w, h), target = the output's (w, h)."""
    (w, h), (tw, th) = size, target
    if pan_direction not in PAN_DIRECTIONS:
        raise ValueError(f"pan_direction must be one of {PAN_DIRECTIONS}, got {pan_direction!r}")
    if total < 1 or tw < 1 or th < 1 or w < tw or h < th:
        raise ValueError(f"the plan needs total >= 1 and a pan size {w}x{h} no smaller than the target {tw}x{th}")
    plan = []
    for g in range(total):
        progress = g / max(1, total - 1)
        nw, nh = w, h
        if zoom_pulse > 0:
            z = calculate_zoom_pulse(progress, zoom_pulse, zoom_pulse_freq)
            nw, nh = int(w * z), int(h * z)
        zoom, pw, ph, cx, cy = extract_pan_geometry(progress, w, h, tw, th, pan_zoom, pan_direction, zoom_in_pct)
        plan.append(CameraFrame(progress, nw, nh, zoom, pw, ph, cx, cy, progress * hue_rotate if hue_rotate != 0 else 0.0))
    return plan


def pan_geometry(w: int, h: int, tw: int, th: int, pan_zoom: float, zoom: float = 1.0) -> Tuple[int, int, int, int, int, int]:
    """load_for_pan (morph_v2.py:715-737): (crop_x, crop_y, crop_w, crop_h, new_w, new_h) -- the optional static
    --zoom centre crop, then the scale max(tw / w, th / h) * pan_zoom to int() sizes; no crop afterwards."""
    x = y = 0
    if zoom > 1.0:
        cw, ch = int(w / zoom), int(h / zoom)
        x, y = (w - cw) // 2, (h - ch) // 2
        w, h = cw, ch
    scale = max(tw / w, th / h) * pan_zoom
    return x, y, w, h, int(w * scale), int(h * scale)


def load_for_pan(path: Path, tw: int, th: int, pan_zoom: float, zoom: float, device: torch.device) -> torch.Tensor:
    """Pillow decode -> RGB -> static zoom crop -> the engine's Pillow-exact LANCZOS to the pan size: uint8
    [new_h,new_w,3] on the device.  The resize REPLACES the reference's cv2.INTER_LANCZOS4, the documented substitution
    morph.load_fitted makes."""
    from PIL import Image

    from .deeplab import Resampler
    with Image.open(path) as im:
        rgb = np.array(im.convert("RGB"), dtype=np.uint8)
    x, y, cw, ch, nw, nh = pan_geometry(rgb.shape[1], rgb.shape[0], tw, th, pan_zoom, zoom)
    t = torch.from_numpy(np.ascontiguousarray(rgb[y:y + ch, x:x + cw])).to(device)[None]
    if (nw, nh) != (cw, ch):
        t = Resampler("lanczos", ch, cw, nh, nw, device)(t)
    return t[0].contiguous()


# ---- Lanczos tables (host, numpy) ----
_S45 = 0.70710678118654752440084436210485
_CS = np.array([[1, 0], [-_S45, -_S45], [0, 1], [_S45, -_S45], [-1, 0], [_S45, _S45], [0, -1], [-_S45, _S45]], np.float64)


def lanczos4_coeffs(fx) -> np.ndarray:
    """OpenCV's interpolateLanczos4(fx) for one fraction ([8]) or an array of them ([n,8]): float32 coefficients
    normalised by their float sum.  sin and cos come from libm (math), one call per fraction, as std::sin would."""
    x = np.atleast_1d(np.asarray(fx, dtype=f32))
    x3 = x + f32(3)
    y0 = -x3.astype(np.float64) * math.pi / 4
    s0 = np.array([math.sin(v) for v in y0], np.float64)
    c0 = np.array([math.cos(v) for v in y0], np.float64)
    co = np.empty((len(x), 8), f32)
    total = np.zeros(len(x), f32)
    for i in range(8):
        d = x3 - f32(i)
        y = -d.astype(np.float64) * math.pi / 4
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            c = ((_CS[i, 0] * s0 + _CS[i, 1] * c0) / (y * y)).astype(f32)
        co[:, i] = np.where(np.abs(d) >= f32(1e-6), c, f32(1e30))
        total = total + co[:, i]
    co = co * (f32(1) / total)[:, None]
    assert co.dtype == f32
    return co[0] if np.ndim(fx) == 0 else co


def lanczos_axis_table(n_src: int, n_dst: int) -> Tuple[np.ndarray, np.ndarray]:
    """(ofs int32 [n_dst], coef int16 [n_dst,8]) of cv2.resize(INTER_LANCZOS4) along one axis: fx = (float)((d + 0.5)
    * scale - 0.5), ofs = floor(fx) (never reset; the kernel clamps each tap), coef = saturate_cast<short>(rint(c *
    2048))."""
    scale = n_src / n_dst
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(f32)
    s = np.floor(f)
    coef = np.clip(np.rint(lanczos4_coeffs((f - s).astype(f32)) * f32(2048)), -32768, 32767).astype(np.int16)
    return s.astype(np.int32), coef


class LanczosTables:
    """Device tables of nst_camera_lanczos_u8 / nst_camera_frames_u8 for a list of crop sizes -> one target: slot i
    belongs to crops[i]."""

    def __init__(self, crops: Sequence[Tuple[int, int]], tw: int, th: int, device: torch.device):
        n = max(1, len(crops))
        xo, xc = np.zeros((n, tw), np.int32), np.zeros((n, tw, 8), np.int16)
        yo, yc = np.zeros((n, th), np.int32), np.zeros((n, th, 8), np.int16)
        axis = {}
        for i, (cw, ch) in enumerate(crops):
            for key in (("x", cw, tw), ("y", ch, th)):
                if key not in axis:
                    axis[key] = lanczos_axis_table(key[1], key[2])
            (xo[i], xc[i]), (yo[i], yc[i]) = axis[("x", cw, tw)], axis[("y", ch, th)]
        self.slots = n
        self.xofs, self.xcoef = torch.from_numpy(xo).to(device), torch.from_numpy(xc).to(device)
        self.yofs, self.ycoef = torch.from_numpy(yo).to(device), torch.from_numpy(yc).to(device)

    def ptrs(self):
        return self.xofs.data_ptr(), self.xcoef.data_ptr(), self.yofs.data_ptr(), self.ycoef.data_ptr()

    def record_stream(self, stream) -> None:
        for t in (self.xofs, self.xcoef, self.yofs, self.ycoef):
            t.record_stream(stream)


# ---- wrappers ----
def _frames(x: torch.Tensor, what: str) -> torch.Tensor:
    _lib.require_gpu_tensor(x, what)
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
        raise NstError(f"{what}: expected a uint8 [n,h,w,3] tensor, got {x.dtype} {tuple(x.shape)}")
    return x.contiguous()


def _ints(v):
    return (ctypes.c_int * len(v))(*[int(a) for a in v])


def _floats(v):
    return (ctypes.c_float * len(v))(*[float(f32(a)) for a in v])


def zoom_pulse_frames(frames_u8: torch.Tensor, sizes: Sequence[Tuple[int, int]]) -> torch.Tensor:
    """(a): frame i resized to sizes[i] = (nw, nh) with INTER_LINEAR and centre-cropped back."""
    x = _frames(frames_u8, "zoom_pulse_frames")
    n, h, w, _ = x.shape
    if len(sizes) != n:
        raise NstError(f"zoom_pulse_frames: {n} frames, {len(sizes)} sizes")
    out = torch.empty_like(x)
    for s in range(0, n, MAX_FRAMES):
        e = min(n, s + MAX_FRAMES)
        check(lib().nst_camera_pulse_u8(x[s:e].data_ptr(), e - s, h, w, _ints([a for a, _ in sizes[s:e]]),
                                        _ints([b for _, b in sizes[s:e]]), out[s:e].data_ptr(),
                                        _lib.stream_ptr(x.device)), "nst_camera_pulse_u8")
    return out


def rect_subpix(frames_u8: torch.Tensor, patch: Tuple[int, int], centres: Sequence[Tuple[float, float]]) -> torch.Tensor:
    """(b): cv2.getRectSubPix(frame i, patch = (pw, ph), centres[i]) -> uint8 [n,ph,pw,3]."""
    x = _frames(frames_u8, "rect_subpix")
    n, h, w, _ = x.shape
    pw, ph = int(patch[0]), int(patch[1])
    if len(centres) != n or pw < 1 or ph < 1:
        raise NstError(f"rect_subpix: {n} frames, {len(centres)} centres, patch {pw}x{ph}")
    out = torch.empty((n, ph, pw, 3), dtype=torch.uint8, device=x.device)
    for s in range(0, n, MAX_FRAMES):
        e = min(n, s + MAX_FRAMES)
        check(lib().nst_camera_rect_subpix_u8(x[s:e].data_ptr(), e - s, h, w, pw, ph, _floats([c[0] for c in centres[s:e]]),
                                              _floats([c[1] for c in centres[s:e]]), out[s:e].data_ptr(),
                                              _lib.stream_ptr(x.device)), "nst_camera_rect_subpix_u8")
    return out


def lanczos_resize(frames_u8: torch.Tensor, crops: Sequence[Tuple[int, int]], target: Tuple[int, int]) -> torch.Tensor:
    """(c): cv2.resize(frame i[:ch, :cw], target = (tw, th), INTER_LANCZOS4) with crops[i] = (cw, ch)."""
    x = _frames(frames_u8, "lanczos_resize")
    n, h, w, _ = x.shape
    tw, th = int(target[0]), int(target[1])
    if len(crops) != n or tw < 1 or th < 1:
        raise NstError(f"lanczos_resize: {n} frames, {len(crops)} crops, target {tw}x{th}")
    for cw, ch in crops:
        if not (1 <= cw <= w and 1 <= ch <= h):
            raise NstError(f"lanczos_resize: crop {cw}x{ch} outside the {w}x{h} frame")
    out = torch.empty((n, th, tw, 3), dtype=torch.uint8, device=x.device)
    for s in range(0, n, MAX_FRAMES):
        e = min(n, s + MAX_FRAMES)
        tab = LanczosTables(crops[s:e], tw, th, x.device)
        check(lib().nst_camera_lanczos_u8(x[s:e].data_ptr(), e - s, h, w, _ints([c[0] for c in crops[s:e]]),
                                          _ints([c[1] for c in crops[s:e]]), tw, th, *tab.ptrs(), out[s:e].data_ptr(),
                                          _lib.stream_ptr(x.device)), "nst_camera_lanczos_u8")
        tab.record_stream(torch.cuda.current_stream(x.device))
    return out


def _hue_args(shifts: Sequence[float]):
    return [0 if abs(s) < 0.1 else 1 for s in shifts], [f32(s / 2) for s in shifts]


def hue_shift_frames(frames_u8: torch.Tensor, shifts: Sequence[float]) -> torch.Tensor:
    """(d): apply_hue_shift(frame i, shifts[i] degrees); |shift| < 0.1 passes through."""
    x = _frames(frames_u8, "hue_shift_frames")
    n, h, w, _ = x.shape
    if len(shifts) != n:
        raise NstError(f"hue_shift_frames: {n} frames, {len(shifts)} shifts")
    out = torch.empty_like(x)
    for s in range(0, n, MAX_FRAMES):
        e = min(n, s + MAX_FRAMES)
        on, half = _hue_args(shifts[s:e])
        check(lib().nst_camera_hue_u8(x[s:e].data_ptr(), e - s, h, w, _ints(on), _floats(half), out[s:e].data_ptr(),
                                      _lib.stream_ptr(x.device)), "nst_camera_hue_u8")
    return out


def smooth_weights(kernel_size: int, sigma: float = 1.0) -> np.ndarray:
    """temporal_smooth_frames' weights, the script's own numpy expression (float64)."""
    half = kernel_size // 2
    weights = np.array([np.exp(-((i - half) ** 2) / (2 * sigma ** 2)) for i in range(kernel_size)])
    return weights / weights.sum()


def temporal_smooth_window(window_u8: torch.Tensor, first: int, seq_len: int, out_first: int, out_count: int,
                           kernel_size: int, sigma: float = 1.0) -> torch.Tensor:
    """(e): smoothed frames out_first .. out_first + out_count - 1 of a sequence of seq_len frames, from the window
    of consecutive frames that starts at global index `first`."""
    x = _frames(window_u8, "temporal_smooth_window")
    n, h, w, _ = x.shape
    if out_count < 1:
        raise NstError("temporal_smooth_window: out_count must be at least 1")
    if not 1 <= kernel_size <= _lib.NST_CAMERA_MAX_SMOOTH:
        raise NstError(f"temporal_smooth_window: kernel_size {kernel_size} outside 1..{_lib.NST_CAMERA_MAX_SMOOTH}")
    wts = np.ascontiguousarray(smooth_weights(kernel_size, sigma), np.float64)
    out = torch.empty((out_count, h, w, 3), dtype=torch.uint8, device=x.device)
    check(lib().nst_camera_smooth_u8(x.data_ptr(), n, h, w, int(first), int(seq_len), int(out_first), int(out_count),
                                     int(kernel_size), wts.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                     out.data_ptr(), _lib.stream_ptr(x.device)), "nst_camera_smooth_u8")
    return out


def temporal_smooth_frames(frames_u8: torch.Tensor, kernel_size: int, sigma: float = 1.0) -> torch.Tensor:
    """The whole sequence at once (the call site's rule: len <= kernel_size, or kernel_size 0, returns it unchanged)."""
    x = _frames(frames_u8, "temporal_smooth_frames")
    n = x.shape[0]
    if kernel_size <= 0 or n <= kernel_size:
        return x.clone()
    return torch.cat([temporal_smooth_window(x, 0, n, s, min(4096, n - s), kernel_size, sigma)
                      for s in range(0, n, 4096)])


def prepare_camera(plan: Sequence[CameraFrame], target: Tuple[int, int], device: torch.device) -> list:
    """The host half of camera_frames: per call of at most MAX_FRAMES frames the descriptor table, the Lanczos tables
    of its zoom-phase crops (on the device) and the scratch."""
    tw, th = int(target[0]), int(target[1])
    calls = []
    for s in range(0, len(plan), MAX_FRAMES):
        chunk = plan[s:s + MAX_FRAMES]
        crops, desc = [], (NstCameraFrame * len(chunk))()
        for i, p in enumerate(chunk):
            on, half = _hue_args([p.hue_shift])
            slot = 0
            if p.zoom:
                if (p.patch_w, p.patch_h) not in crops:
                    crops.append((p.patch_w, p.patch_h))
                slot = crops.index((p.patch_w, p.patch_h))
            desc[i] = NstCameraFrame(int(p.pulse_w), int(p.pulse_h), int(bool(p.zoom)), int(p.patch_w), int(p.patch_h),
                                     float(f32(p.cx)), float(f32(p.cy)), on[0], float(half[0]), slot)
        sz = ctypes.c_size_t()
        check(lib().nst_camera_scratch_bytes(desc, len(chunk), ctypes.byref(sz)), "nst_camera_scratch_bytes")
        tab = LanczosTables(crops, tw, th, device) if crops else None
        scratch = torch.empty((max(sz.value, 16),), dtype=torch.uint8, device=device)
        calls.append((s, len(chunk), desc, tab, scratch, sz.value))
    return calls


def run_camera(frames_u8: torch.Tensor, calls: list, target: Tuple[int, int]) -> torch.Tensor:
    """The device half: at most two launches per prepared call."""
    x = _frames(frames_u8, "camera_frames")
    n, h, w, _ = x.shape
    tw, th = int(target[0]), int(target[1])
    if sum(c[1] for c in calls) != n:
        raise NstError(f"camera_frames: {n} frames, {sum(c[1] for c in calls)} plan entries")
    out = torch.empty((n, th, tw, 3), dtype=torch.uint8, device=x.device)
    stream = torch.cuda.current_stream(x.device)
    for s, m, desc, tab, scratch, need in calls:
        ptrs = tab.ptrs() if tab else (None, None, None, None)
        check(lib().nst_camera_frames_u8(x[s:s + m].data_ptr(), m, h, w, desc, tw, th, *ptrs, tab.slots if tab else 0,
                                         out[s:s + m].data_ptr(), scratch.data_ptr(), need, _lib.stream_ptr(x.device)),
              "nst_camera_frames_u8")
        scratch.record_stream(stream)
        if tab:
            tab.record_stream(stream)
    return out


def camera_frames(frames_u8: torch.Tensor, plan: Sequence[CameraFrame], target: Tuple[int, int]) -> torch.Tensor:
    """(f): morph frames [n,h,w,3] through their plan entries -> uint8 [n,th,tw,3]; MAX_FRAMES frames per call, two
    launches each (one when no frame is in the zoom phase)."""
    x = _frames(frames_u8, "camera_frames")
    if len(plan) != x.shape[0]:
        raise NstError(f"camera_frames: {x.shape[0]} frames, {len(plan)} plan entries")
    return run_camera(x, prepare_camera(plan, target, x.device), target)


class SmoothStream:
    """temporal_smooth_frames over a sequence that arrives in batches: push() camera frames in order, get back the
    smoothed frames whose taps are all there; kernel_size // 2 frames of halo are carried between batches, never the
    whole video.  kernel_size 0, or a sequence no longer than the kernel, passes frames through (the call site's
    condition)."""

    def __init__(self, total: int, kernel_size: int, sigma: float = 1.0):
        self.total, self.k, self.sigma = int(total), int(kernel_size), sigma
        self.on = self.k > 0 and self.total > self.k
        self.half = self.k // 2
        self.ahead = self.k - 1 - self.half if self.on else 0  # taps after the output frame
        self.win: Optional[torch.Tensor] = None
        self.first = 0   # global index of win[0]
        self.have = 0    # frames pushed so far
        self.done = 0    # frames returned so far

    def push(self, frames_u8: torch.Tensor) -> Optional[torch.Tensor]:
        self.have += frames_u8.shape[0]
        if self.have > self.total:
            raise NstError(f"SmoothStream: {self.have} frames pushed into a sequence of {self.total}")
        if not self.on:
            self.done = self.have
            return frames_u8
        self.win = frames_u8 if self.win is None else torch.cat([self.win, frames_u8])
        ready = self.have if self.have == self.total else self.have - self.ahead  # outputs < ready are computable
        if ready <= self.done:
            return None
        out = temporal_smooth_window(self.win, self.first, self.total, self.done, ready - self.done, self.k, self.sigma)
        self.done = ready
        keep = max(self.first, self.done - self.half)
        self.win = self.win[keep - self.first:]
        self.first = keep
        return out
