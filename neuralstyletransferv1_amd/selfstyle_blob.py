"""Selfstyle blob video on the MI355X engine: the reference's animated soft-blob compositor
(scripts/selfstyle_blob.py, generate_blob_video) over the tile/overlap stills its self-style stage writes
(`<name>_tile256_overlap32.jpg`, ...).

Each of up to 8 blobs walks through the stills at its own phase, cross-fading neighbours; a sine-noise field per blob
(4 octaves of a row, a column and a diagonal term, drifting with the frame number) goes through a softmax with
temperature max(0.1, 5 * feather) and weighs the blobs' images per pixel.  With --magenta_dir (the script's
--mix_styles) the odd blobs walk through a second set of stills.  The reference evaluates this with a Python loop over
whole-frame numpy arrays; here

  plan()          the script's scalars per frame, in double: the time terms and, per blob, two stills and their weights
  field()         what a video keeps for all frames: frequencies, amplitudes, the legacy-generator phases, T
  blob_frames()   nst_blob_frames: masks, cross-fades and the weighted sum in one pass over the u8 stills
  blob_masks()    nst_blob_masks: the weights alone (what scripts/morph_faces.py's blob_face_morph takes; feather 0.3)

The arithmetic is the reference's numpy float32 code under the NumPy it pins (< 2.0: every Python scalar rounded to
fp32 once, every operation float32).  sin and exp come from the GPU's maths library, so masks agree with numpy's to
within the distance two CPU libraries have from each other and frames to within one grey level on a small share of the
bytes; one blob is byte-exact.  tests/blob_ref.py is the numpy yardstick.  Restated, parity unpinned
(cv2 is not installed here): cv2.imread is Pillow's decode, cv2.resize is the cv_linear resampler, cv2.addWeighted is
nst_add_weighted_u8.

Not built: stills of mixed sizes (the script resizes inside get_blended_image, after a blend: a different order; here
every still must have the first still's size); the script's Magenta self-style stage and its PyTorch-on-top stage
(the CLI consumes existing stills, the script's --skip_styling path); cv2's VideoWriter and the H.264 re-encode
(assemble_video stands in, as in the sibling CLIs).
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, stills
from ._lib import NstError, check, lib
from .stills import UsageError, header_size

FEATHER = 0.15      # the script's fixed feather (scripts/morph_faces.py passes 0.3)
SEED_STEP = 1000    # blob b's phases come from seed + 1000 * b


# ---- the script's scalars ----
def _overlaps(tile: int) -> List[int]:
    """The overlaps the self-style stage tries at one tile size: tile // 8 (at least 16), tile // 3 where that is
    larger, and between them, where they lie more than 8 apart, their midpoint rounded down to a multiple of 8."""
    low, high = max(16, tile // 8), tile // 3
    mid = (low + high) // 2 // 8 * 8
    between = [mid] if high > low + 8 and mid != low else []
    return [low] + between + ([high] if high > low else [])


def generate_tile_configs(min_tile: int = 256, max_tile: int = 512, num_styles: int = 24) -> List[Tuple[int, int]]:
    """The (tile, overlap) pairs the script's self-style stage runs, in its order: tile sizes from min_tile up in
    steps of a third of num_styles to the range (at least 4 sizes, at least 16 apart), the first num_styles pairs."""
    step = max(16, (max_tile - min_tile) // max(4, num_styles // 3))
    pairs = [(tile, ov) for tile in range(min_tile, max_tile + 1, step) for ov in _overlaps(tile)]
    return pairs[:num_styles]


def sort_key(p) -> Tuple[int, int]:
    """(tile, overlap) from the `tileN` and `overlapN` parts of a still's name, the last of each kind, 0 for a kind the
    name lacks; a part that is not a number raises ValueError, as in the script."""
    parts = Path(p).stem.split("_")
    numbers = {word: [int(q.replace(word, "")) for q in parts if q.startswith(word)] for word in ("tile", "overlap")}
    return tuple(v[-1] if v else 0 for v in numbers.values())


def phases(seed: int, n_blobs: int) -> np.ndarray:
    """float64 [n_blobs, 4, 3]: per blob and octave the script's (phase_x, phase_y, phase_t), from the legacy generator
    seeded with seed + 1000 * blob (np.random.seed, then 12 np.random.random() draws), each times 2 pi."""
    out = np.empty((n_blobs, 4, 3), np.float64)
    for b in range(n_blobs):
        rs = np.random.RandomState(seed + b * SEED_STEP)  # the stream np.random.seed gives, without the global state
        for o in range(4):
            for k in range(3):
                out[b, o, k] = rs.random_sample() * 2 * np.pi
    return out


def field(n_blobs: int, frequency: float = 2.5, seed: int = 42, feather: float = FEATHER) -> dict:
    """What the masks of a video keep for all frames, in doubles (the struct rounds each to fp32 once)."""
    if not 1 <= n_blobs <= _lib.NST_BLOB_MAX:
        raise NstError(f"selfstyle_blob: {n_blobs} blobs outside 1..{_lib.NST_BLOB_MAX}")
    ph = phases(seed, n_blobs)
    amp = [1.0 / (1.5 ** o) for o in range(4)]
    return dict(n_blobs=n_blobs, T=max(0.1, feather * 5), freq=[frequency * (2 ** o) for o in range(4)], amp=amp,
                amp_half=[a * 0.5 for a in amp], phase_x=ph[:, :, 0].tolist(), phase_y=ph[:, :, 1].tolist(),
                phase_t=ph[:, :, 2].tolist(), blob_phase=[b * 2 * np.pi / n_blobs for b in range(n_blobs)])


def frame_times(frame_idx: int, speed: float = 1.0) -> dict:
    """The three drift terms of frame frame_idx."""
    time_offset = frame_idx * speed * 0.02
    return dict(t_y=[time_offset * (1 + o * 0.3) for o in range(4)], t_x=[time_offset * (1.2 + o * 0.2) for o in range(4)],
                t_t=time_offset * 1.5)


def plan(n_styled: int, n_magenta: int = 0, fps: int = 24, duration: int = 30, num_blobs: int = 2,
         transition_speed: float = 1.0, blob_speed: float = 1.0) -> List[dict]:
    """The script's frame loop in Python doubles: one descriptor per output frame, the drift terms and per blob the
    two stills get_blended_image cross-fades and their weights.  Bank indices: the styled stills 0..n_styled-1, then
    the magenta-only ones; with n_magenta > 0 the odd blobs walk through those."""
    if n_styled < 1:
        raise NstError("selfstyle_blob: no styled stills")
    total_frames = fps * duration
    out = []
    for frame_idx in range(total_frames):
        t = frame_idx / total_frames
        d = frame_times(frame_idx, blob_speed)
        blobs = []
        for b in range(num_blobs):
            base, n = (n_styled, n_magenta) if (n_magenta and b % 2 == 1) else (0, n_styled)
            pos = (t * transition_speed * (n - 1) + (b / num_blobs) * n) % n  # get_blended_image's own % n changes nothing
            idx1 = int(pos)
            idx2 = (idx1 + 1) % n
            blend = pos - idx1
            blobs.append(dict(lo=base + idx1, hi=base + idx2, w_lo=1 - blend, w_hi=blend))
        d["blobs"] = blobs
        out.append(d)
    return out


def output_size(w: int, h: int, max_resolution: int) -> Tuple[int, int]:
    """(width, height) of the video: the longest edge capped at max_resolution, both edges made even."""
    if max(h, w) > max_resolution:
        scale = max_resolution / max(h, w)
        return int(w * scale) - (int(w * scale) % 2), int(h * scale) - (int(h * scale) % 2)
    return w - (w % 2), h - (h % 2)


# ---- device ----
def pack_field(fd: dict):
    """The field as nst_blob_field (doubles rounded to fp32 here, once)."""
    a = _lib.NstBlobField()
    a.n_blobs, a.T = int(fd["n_blobs"]), float(fd["T"])
    for o in range(4):
        a.freq[o], a.amp[o], a.amp_half[o] = float(fd["freq"][o]), float(fd["amp"][o]), float(fd["amp_half"][o])
    for b in range(min(len(fd["blob_phase"]), _lib.NST_BLOB_MAX)):
        for o in range(4):
            a.phase_y[b][o], a.phase_x[b][o] = float(fd["phase_y"][b][o]), float(fd["phase_x"][b][o])
            a.phase_t[b][o] = float(fd["phase_t"][b][o])
        a.blob_phase[b] = float(fd["blob_phase"][b])
    return a


def pack(descs: Sequence[dict]):
    """The plan's descriptors as an array of nst_blob_frame (doubles rounded to fp32 here, once)."""
    arr = (_lib.NstBlobFrame * len(descs))()
    for a, d in zip(arr, descs):
        if len(d["blobs"]) > _lib.NST_BLOB_MAX:
            raise NstError(f"selfstyle_blob: a frame has at most {_lib.NST_BLOB_MAX} blobs, got {len(d['blobs'])}")
        for o in range(4):
            a.t_y[o], a.t_x[o] = float(d["t_y"][o]), float(d["t_x"][o])
        a.t_t = float(d["t_t"])
        for b, s in enumerate(d["blobs"]):
            a.blob[b].lo, a.blob[b].hi = int(s["lo"]), int(s["hi"])
            a.blob[b].w_lo, a.blob[b].w_hi = float(s["w_lo"]), float(s["w_hi"])
    return arr


def norm_tables(h: int, w: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """(yn, xn): np.linspace(0, 1, h or w, dtype=float32) on the device, uploaded once per video."""
    return (torch.from_numpy(np.linspace(0, 1, h, dtype=np.float32)).to(device),
            torch.from_numpy(np.linspace(0, 1, w, dtype=np.float32)).to(device))


def _check_tables(who: str, yn: torch.Tensor, xn: torch.Tensor, h: int, w: int) -> None:
    for name, t, n in (("yn", yn, h), ("xn", xn, w)):
        _lib.require_gpu_tensor(t, f"{who} {name}")
        if t.dtype != torch.float32 or tuple(t.shape) != (n,) or not t.is_contiguous():
            raise NstError(f"{who}: expected a contiguous float32 [{n}] {name}, got {t.dtype} {tuple(t.shape)}")


def blob_frames(bank_u8: torch.Tensor, yn: torch.Tensor, xn: torch.Tensor, fd: dict,
                descs: Sequence[dict]) -> torch.Tensor:
    """bank uint8 [n_bank,h,w,3] on the device, the tables of norm_tables(), a field() and descriptors as plan() emits
    them -> uint8 [n,h,w,3]."""
    if isinstance(bank_u8, torch.Tensor) and bank_u8.dim() == 4:
        _check_tables("blob_frames", yn, xn, bank_u8.shape[1], bank_u8.shape[2])
    fld = pack_field(fd)
    out = stills.bank_frames("blob_frames", "nst_blob_frames", pack, bank_u8, descs,
                             (yn.data_ptr(), xn.data_ptr(), fld))
    for t in (yn, xn):
        t.record_stream(torch.cuda.current_stream(t.device))
    return out


def blob_masks(h: int, w: int, yn: torch.Tensor, xn: torch.Tensor, fd: dict, descs: Sequence[dict]) -> torch.Tensor:
    """The softmax weights alone: float32 [n, n_blobs, h, w] on the tables' device (a descriptor's stills are not
    read: frame_times() alone is a descriptor here)."""
    _check_tables("blob_masks", yn, xn, h, w)
    n, nb = len(descs), int(fd["n_blobs"])
    frames = pack([dict(d, blobs=()) for d in descs])
    if not 1 <= nb <= _lib.NST_BLOB_MAX:
        raise NstError(f"blob_masks: {nb} blobs outside 1..{_lib.NST_BLOB_MAX}")
    out = torch.empty((max(n, 0), nb, h, w), dtype=torch.float32, device=yn.device)
    check(lib().nst_blob_masks(h, w, yn.data_ptr(), xn.data_ptr(), pack_field(fd), frames, n, out.data_ptr(),
                               _lib.stream_ptr(yn.device)), "nst_blob_masks")
    for t in (yn, xn):
        t.record_stream(torch.cuda.current_stream(t.device))
    return out


def add_weighted_u8(a: torch.Tensor, wa: float, b: torch.Tensor, wb: float) -> torch.Tensor:
    """cv2.addWeighted(a, wa, b, wb, 0) of two uint8 tensors of one shape on the device."""
    _lib.require_gpu_tensor(a, "add_weighted_u8 a")
    _lib.require_gpu_tensor(b, "add_weighted_u8 b")
    if a.dtype != torch.uint8 or b.dtype != torch.uint8 or a.shape != b.shape:
        raise NstError(f"add_weighted_u8: expected two uint8 tensors of one shape, got {a.dtype} {tuple(a.shape)} and "
                       f"{b.dtype} {tuple(b.shape)}")
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty_like(a)
    check(lib().nst_add_weighted_u8(a.data_ptr(), float(wa), b.data_ptr(), float(wb), a.numel(), out.data_ptr(),
                                    _lib.stream_ptr(a.device)), "nst_add_weighted_u8")
    for t in (a, b):
        t.record_stream(torch.cuda.current_stream(t.device))
    return out


def _as_is(w: int, h: int):
    return None, (w, h)


def load_and_blend(paths: Sequence, original, blend_original: float, device=None,
                   jpeg_reader: str = "pil") -> torch.Tensor:
    """The script's load_and_blend over stills of one size: uint8 [len(paths),h,w,3] on the device, each still blended
    with the original (resized to the stills' size with cv2.resize's default, bilinear) when blend_original > 0."""
    from .deeplab import Resampler
    device = torch.device(device or "cuda:0")
    bank = stills.load_bank(paths, _as_is, device, jpeg_reader)
    if not blend_original > 0:
        return bank
    orig = stills.load_bank([original], _as_is, device, jpeg_reader)
    h, w = bank.shape[1:3]
    if tuple(orig.shape[1:3]) != (h, w):
        orig = Resampler("cv_linear", orig.shape[1], orig.shape[2], h, w, device)(orig)
    return torch.stack([add_weighted_u8(img, 1 - blend_original, orig[0], blend_original) for img in bank])


# ---- CLI ----
def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m neuralstyletransferv1_amd.selfstyle_blob",
                                 description="Animated soft-blob compositor over pre-styled stills on the GPU")
    ap.add_argument("--styled_dir", type=str, required=True, help="directory of the *_tile*_overlap*.jpg stills")
    ap.add_argument("--original", type=str, required=True, help="the image the stills were styled from")
    ap.add_argument("--magenta_dir", type=str, default=None,
                    help="a second directory of stills for the odd blobs (the script's --mix_styles)")
    ap.add_argument("--output", type=str, default=None, help="also assemble the frames into this video with ffmpeg")
    ap.add_argument("--fps", type=int, default=24)
    ap.add_argument("--duration", type=int, default=30, help="seconds")
    ap.add_argument("--blend_original", type=float, default=0.5, help="0 = the stills alone, 1 = the original alone")
    ap.add_argument("--blob_frequency", type=float, default=2.5)
    ap.add_argument("--blob_speed", type=float, default=1.0)
    ap.add_argument("--max_resolution", type=int, default=1280, help="longest edge of the output")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--num_blobs", type=int, default=2, help="1..8")
    ap.add_argument("--transition_speed", type=float, default=1.0)
    ap.add_argument("--feather", type=float, default=FEATHER, help="softmax temperature / 5 (the script fixes 0.15)")
    stills.add_output_flags(ap, "blob_frame")
    ap.add_argument("--jpeg_reader", choices=["pil", "gpu"], default="pil")
    ap.add_argument("--batch", type=int, default=8, help="output frames per kernel call")
    ap.add_argument("--device", type=str, default="cuda:0")
    return ap


def find_stills(directory) -> List[Path]:
    """The script's --skip_styling listing: *_tile*_overlap*.jpg, by name, then (stably) by (tile, overlap)."""
    found = sorted(Path(directory).glob("*_tile*_overlap*.jpg"))
    try:
        return sorted(found, key=sort_key)
    except ValueError as e:
        raise UsageError(f"{directory}: a still's tile or overlap is not a number ({e})")


def prepare(args) -> Tuple[List[Path], List[Path], Tuple[int, int], Tuple[int, int]]:
    """Everything the CLI decides before it touches the device: (styled stills, magenta stills, (w, h) of the stills,
    (w, h) of the output); UsageError for the exit-2 cases.  Only image headers are read."""
    if args.fps < 1 or args.duration < 1 or args.batch < 1 or args.max_resolution < 2:
        raise UsageError("need --fps, --duration, --batch >= 1 and --max_resolution >= 2")
    if not 1 <= args.num_blobs <= _lib.NST_BLOB_MAX:
        raise UsageError(f"--num_blobs {args.num_blobs} outside 1..{_lib.NST_BLOB_MAX}")
    if not 0 <= args.seed <= 2 ** 32 - 1 - SEED_STEP * (_lib.NST_BLOB_MAX - 1):
        raise UsageError("--seed: the legacy generator takes seeds 0..2^32-1, and blob b uses seed + 1000 b")
    if not 0 <= args.blend_original <= 1:
        raise UsageError("--blend_original outside 0..1")
    sizes = {}

    def readable(directory) -> List[Path]:  # a still that does not load is skipped, as the script's load_and_blend does
        keep = []
        for p in find_stills(directory):
            sizes[p] = header_size(p)
            if sizes[p] is not None:
                keep.append(p)
        return keep

    styled = readable(args.styled_dir)
    if not styled:
        raise UsageError(f"no readable *_tile*_overlap*.jpg stills in {args.styled_dir}")
    magenta = readable(args.magenta_dir) if args.magenta_dir else []
    if header_size(Path(args.original)) is None:
        raise UsageError(f"{args.original}: not a readable image")
    size = None
    for p in styled + magenta:
        got = sizes[p]
        if size is None:
            size = got
        elif got != size:
            raise UsageError(f"{p}: is {got[0]}x{got[1]}, {styled[0]} is {size[0]}x{size[1]} (stills of mixed sizes "
                             "are not built)")
    out_wh = output_size(size[0], size[1], args.max_resolution)
    if out_wh[0] < 2 or out_wh[1] < 2:
        raise UsageError(f"{size[0]}x{size[1]} stills give a {out_wh[0]}x{out_wh[1]} video")
    return styled, magenta, size, out_wh


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = build_parser().parse_args(argv)
    try:
        styled, magenta, (w, h), (ow, oh) = prepare(args)
    except UsageError as e:
        print(f"[selfstyle_blob] {e}", file=sys.stderr)
        return 2
    from .deeplab import Resampler
    device = torch.device(args.device)
    wr = stills.open_writer(args)
    bank = load_and_blend(styled + magenta, args.original, args.blend_original, device, args.jpeg_reader)
    yn, xn = norm_tables(h, w, device)
    fd = field(args.num_blobs, args.blob_frequency, args.seed, args.feather)
    pl = plan(len(styled), len(magenta), args.fps, args.duration, args.num_blobs, args.transition_speed,
              args.blob_speed)
    resize = Resampler("cv_linear", h, w, oh, ow, device) if (ow, oh) != (w, h) else None
    print(f"[selfstyle_blob] {len(pl)} frames, {args.num_blobs} blobs over {len(styled)} styled"
          f"{f' and {len(magenta)} magenta-only' if magenta else ''} stills at {w}x{h}, written at {ow}x{oh}")
    for s in range(0, len(pl), args.batch):  # streamed: a batch is written before the next is computed
        frames = blob_frames(bank, yn, xn, fd, pl[s:s + args.batch])
        wr.write(resize(frames) if resize is not None else frames)
    stills.close_run("selfstyle_blob", wr, args.fps, args.output)
    return 0


if __name__ == "__main__":
    sys.exit(main())
