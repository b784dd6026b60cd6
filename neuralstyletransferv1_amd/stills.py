"""What the still compositors' CLIs (morph, style_morph, multi_model_video, selfstyle_blob) share around their kernels: the output
flags and the numbered-file writer, the close of a run, the two easing curves, the ctypes call of a bank kernel
(csrc/u8run_common.h, launch_bank_frames) and the loader of a bank of stills.

The loader is the reference scripts' load_resize over a list of files: Pillow's decode to RGB stands for cv2.imread,
camera.lanczos_resize for cv2.resize(INTER_LANCZOS4), parity unpinned (cv2 is not installed here).  What differs
between the scripts is their fit rule, which the caller passes in.
"""
from __future__ import annotations

import argparse
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import NstError, check, lib
from .pipeline import assemble_video

# fit(w, h) of a decoded w x h source -> ((x, y, cw, ch) to crop first or None, (tw, th) to resize to); it raises
# NstError (the loader puts the file's path in front) for a source it cannot fit
FitRule = Callable[[int, int], Tuple[Optional[Tuple[int, int, int, int]], Tuple[int, int]]]


class UsageError(Exception):
    """A condition the CLI reports with exit status 2 before it touches the device."""


def ease_in_out_cubic(t: float) -> float:
    return 4 * t * t * t if t < 0.5 else 1 - pow(-2 * t + 2, 3) / 2


def smoothstep(t: float) -> float:
    return t * t * (3 - 2 * t)


def header_size(path: Path) -> Optional[Tuple[int, int]]:
    """(width, height) from the image's header, None for a file Pillow cannot read (cv2.imread returns None for such
    a file and the scripts then skip it)."""
    from PIL import Image
    try:
        with Image.open(path) as im:
            return im.size
    except Exception:
        return None


# ---- output ----
class FrameWriter:
    """Numbered files {prefix}_{0001..}.{ext} through the frame loop's writers."""

    def __init__(self, out_dir: Path, prefix: str, ext: str, quality: int, png_writer: str, jpeg_writer: str):
        self.dir, self.prefix, self.ext, self.quality = out_dir, prefix, ext, int(quality)
        self.png_writer, self.jpeg_writer = png_writer, jpeg_writer
        self.count = 0

    def write(self, frames_u8: torch.Tensor) -> None:
        from PIL import Image
        blobs = None
        if self.ext == "jpg" and self.jpeg_writer == "gpu":
            from .jpegio import jpeg_bytes_gpu
            blobs = jpeg_bytes_gpu(frames_u8, self.quality)
        elif self.ext == "png" and self.png_writer == "gpu":
            from .pngio import png_bytes_gpu
            blobs = png_bytes_gpu(frames_u8)
        host = None if blobs is not None else frames_u8.cpu().numpy()
        for j in range(frames_u8.shape[0]):
            self.count += 1
            path = self.dir / f"{self.prefix}_{self.count:04d}.{self.ext}"
            if blobs is not None:
                path.write_bytes(blobs[j])
            elif self.ext == "jpg":
                Image.fromarray(host[j]).save(path, format="JPEG", quality=self.quality)
            elif self.png_writer == "fast":
                from .pngio import write_png
                write_png(path, host[j])
            else:
                Image.fromarray(host[j]).save(path)


def add_output_flags(ap: argparse.ArgumentParser, prefix: str) -> None:
    """The six flags of the frame files; `prefix` is the CLI's default --output_prefix."""
    ap.add_argument("--output_dir", type=str, required=True)
    ap.add_argument("--output_prefix", type=str, default=prefix)
    ap.add_argument("--image_ext", choices=["png", "jpg"], default="png")
    ap.add_argument("--jpeg_quality", type=int, default=85)
    ap.add_argument("--png_writer", choices=["fast", "pil", "gpu"], default="pil")
    ap.add_argument("--jpeg_writer", choices=["pil", "gpu"], default="pil")


def open_writer(args) -> FrameWriter:
    """--output_dir made, and the writer the six flags describe."""
    out_dir = Path(args.output_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    return FrameWriter(out_dir, args.output_prefix, args.image_ext, args.jpeg_quality, args.png_writer, args.jpeg_writer)


def close_run(tag: str, wr: FrameWriter, fps, video: Optional[str]) -> None:
    """The end of a CLI run: the frames assembled into `video` with ffmpeg if one was asked for, and the count line."""
    if video:
        assemble_video(wr.dir, Path(video), fps, None, wr.prefix)
    print(f"[{tag}] wrote {wr.count} frames to {wr.dir}")


# ---- device ----
def bank_frames(who: str, entry: str, pack: Callable, bank_u8: torch.Tensor, descs: Sequence[dict],
                extra: Sequence = ()) -> torch.Tensor:
    """A bank call: bank uint8 [n_bank,h,w,3] on the device and the plan's descriptors -> uint8 [n,h,w,3] through the
    C entry point `entry`, the descriptors packed by pack(); `who` is the calling wrapper's name in the messages.
    `extra`: what the entry point takes between w and the descriptors (nst_blob_frames: its tables and its field)."""
    _lib.require_gpu_tensor(bank_u8, f"{who} bank")
    if bank_u8.dtype != torch.uint8 or bank_u8.dim() != 4 or bank_u8.shape[3] != 3:
        raise NstError(f"{who}: expected a uint8 [n_bank,h,w,3] bank, got {bank_u8.dtype} {tuple(bank_u8.shape)}")
    bank = bank_u8.contiguous()
    n_bank, h, w, _ = bank.shape
    n = len(descs)
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=bank.device)
    check(getattr(lib(), entry)(bank.data_ptr(), n_bank, h, w, *extra, pack(descs), n, out.data_ptr(),
                                _lib.stream_ptr(bank.device)), entry)
    bank.record_stream(torch.cuda.current_stream(bank.device))
    return out


def _decode_pil(path) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"), dtype=np.uint8)


def _decode(paths: Sequence, device: torch.device, jpeg_reader: str) -> List[torch.Tensor]:
    """Every file as uint8 [h,w,3] on the device: Pillow on a thread pool, or, jpeg_reader "gpu", jpegio.decode_gpu
    per geometry with Pillow for the files off its fast path."""
    n = len(paths)
    decoded: List[Optional[torch.Tensor]] = [None] * n
    todo = list(range(n))
    with ThreadPoolExecutor(max_workers=min(16, n)) as pool:
        if jpeg_reader == "gpu":
            from . import jpegio
            blobs = list(pool.map(lambda p: Path(p).read_bytes(), paths))
            groups: Dict[tuple, List[int]] = {}
            for i, b in enumerate(blobs):
                info = jpegio.probe(b)
                if info is not None:
                    groups.setdefault(info, []).append(i)
            for idx in groups.values():
                try:
                    frames = jpegio.decode_gpu([blobs[i] for i in idx], device)
                except NstError:  # a damaged stream among them: Pillow decides, file by file
                    continue
                for i, fr in zip(idx, frames):
                    decoded[i] = fr
            todo = [i for i in todo if decoded[i] is None]
        for i, rgb in zip(todo, pool.map(_decode_pil, [paths[i] for i in todo])):
            decoded[i] = torch.from_numpy(rgb).to(device)
    return decoded


def load_bank(paths: Sequence, fit: FitRule, device=None, jpeg_reader: str = "pil") -> torch.Tensor:
    """The files of `paths`, each cropped and resized as fit() says, all to one size: uint8 [len(paths),h,w,3] on the
    device.  One camera.lanczos_resize call per source geometry; a source already at the target size is copied."""
    from .camera import lanczos_resize
    device = torch.device(device or "cuda:0")
    n = len(paths)
    if n == 0:
        raise NstError("load_bank: no files")
    decoded = _decode(paths, device, jpeg_reader)
    target = None
    by_geometry: Dict[Tuple[int, int], Tuple[Optional[Tuple[int, int, int, int]], List[int]]] = {}
    for i, t in enumerate(decoded):
        h, w = t.shape[:2]
        try:
            crop, wh = fit(w, h)
        except NstError as e:
            raise NstError(f"{paths[i]}: {e}")
        if target is None:
            target = wh
        elif wh != target:
            raise NstError(f"{paths[i]}: loads at {wh[0]}x{wh[1]}, {paths[0]} at {target[0]}x{target[1]}")
        by_geometry.setdefault((w, h), (crop, []))[1].append(i)
    bank = torch.empty((n, target[1], target[0], 3), dtype=torch.uint8, device=device)
    for (w, h), (crop, idx) in by_geometry.items():
        x, y, cw, ch = crop or (0, 0, w, h)
        src = torch.stack([decoded[i][y:y + ch, x:x + cw] for i in idx])
        bank[idx] = src if (cw, ch) == target else lanczos_resize(src, [(cw, ch)] * len(idx), target)
    return bank
