"""Multi-model video on the MI355X engine: the reference's pulsed multi-style compositor
(scripts/multi_model_video.py) over the ladder stills the stylizer writes per extracted frame
(`frame_0017_udnie_style5e10.jpg`, ... beside `frame_0017_original.jpg`, and a `walk_<style>.json` naming the rungs).

An original intro, a styled section and an original outro.  The styled section ramps slowly through the udnie ladder,
interweaves mosaic (rung 0) and tenharmsel (rung 5) with offset Gaussian pulses, boosts the saturation and fades in
from the original over its first frames; each section cross-fades into the next, and every source frame is written
hold_frames times.  The reference loops over float32 numpy frames and truncates to u8 between its stages; here

  plan()                  the script's scalars, in double, and its file checks, per source frame -> the distinct files
                          the frame reads, one descriptor over them, the hold count
  multi_model_frames()    nst_multi_model_frames: every stage of a frame in one pass over the u8 stills

The arithmetic is the reference's own numpy float32 code (each Python scalar rounded to fp32 once, every product and
sum on its own, every truncation where the script has it), so frames equal the script's byte for byte given the same
stills.  What is restated, parity unpinned (cv2 is not installed here): cv2.imread is Pillow's decode, the fit is
camera.lanczos_resize (INTER_LANCZOS4), and adjust_saturation's two cvtColor calls are the camera stage's 8-bit HSV
conversions.  tests/multi_model_ref.py is the numpy yardstick.

The script's quirks are kept: the walk file's `walk` list is smoothed there and never read, so only `weights` is
taken; the cross-fade compares source frames against the output-frame count; the intro cross-fades into the udnie
directory's copy of the original (a blend that truncation does not leave the identity); --portrait is always on.

Out of scope (not built): cv2's VideoWriter and the H.264 re-encode (assemble_video replaces them),
style_video_pipeline.py's orchestration, parity with OpenCV itself.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from datetime import datetime
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib, stills
from ._lib import NstError
from .stills import UsageError, header_size, smoothstep

STYLES = ("udnie", "mosaic", "tenharmsel")
MOSAIC_DEFAULT = ("mosaic_style5e10",)  # the script's ladder for a mosaic directory without a walk file
TENHARMSEL_POS = 5                      # the rung the script takes tenharmsel at
SMOOTHNESS = 0.05                       # the script's EMA over `walk`; logged, never used


# ---- the script's scalars ----
def fitted_size(w: int, h: int, size: int = 1080, portrait: bool = True) -> Tuple[int, int]:
    """(width, height) load_resize gives a w x h source: portrait scales the width to `size`, otherwise the longer
    side."""
    if portrait:
        return size, int(h * (size / w))
    scale = size / w if w > h else size / h
    return int(w * scale), int(h * scale)


def gaussian_pulse(t: float, num_pulses: int = 4, width: float = 0.15) -> float:
    total = 0
    for i in range(num_pulses):
        center = (i + 0.5) / num_pulses
        total += math.exp(-((t - center) ** 2) / (2 * width ** 2))
    return min(1.0, total)


def ramp_position(src_idx: int, segment_frames: int, n_weights: int) -> float:
    """The slow step-wise ramp: weight position of source frame src_idx of a styled section."""
    frames_per_weight = max(1, segment_frames // n_weights)
    weight_idx = min(src_idx // frames_per_weight, n_weights - 1)
    weight_progress = (src_idx % frames_per_weight) / frames_per_weight
    return weight_idx + weight_progress * 0.5


def pulse_blends(segment_progress: float) -> Tuple[float, float]:
    """(mosaic_blend, tenharmsel_blend) at a section progress of 0..1."""
    return (gaussian_pulse(segment_progress, num_pulses=4, width=0.10) * 0.5,
            gaussian_pulse(segment_progress + 0.125, num_pulses=4, width=0.10) * 0.5)


# ---- walk files ----
def find_walk(style_dir, style: str) -> Optional[Path]:
    """walk_<style>.json, then walk.json."""
    for name in (f"walk_{style}.json", "walk.json"):
        p = Path(style_dir) / name
        if p.exists():
            return p
    return None


def load_weights(styled_dirs: Dict[str, str]) -> Dict[str, List[str]]:
    """{style: the `weights` list of its walk file} for the directories that have one."""
    weights = {}
    for style, d in styled_dirs.items():
        p = find_walk(d, style)
        if p is None:
            continue
        try:
            with open(p) as f:
                wts = json.load(f)["weights"]
        except (OSError, ValueError, KeyError, TypeError) as e:
            raise UsageError(f"{p}: no readable `weights` list ({type(e).__name__})")
        if not isinstance(wts, list):
            raise UsageError(f"{p}: `weights` is not a list")
        weights[style] = [str(w) for w in wts]
    return weights


# ---- the plan ----
def _styled_still(styled_dir: Path, frame_name: str, weights: Sequence[str], weight_pos: float, orig_blend: float,
                  readable: Callable, exists: Callable) -> Optional[dict]:
    """get_styled_frame without the pixels: None when the directory's original is missing, else the paths ST reads
    and its weights (lo None: the original alone; hi None: one rung)."""
    orig = styled_dir / f"{frame_name}_original.jpg"
    if not readable(orig):
        return None
    idx_low = int(weight_pos)
    idx_high = min(idx_low + 1, len(weights) - 1)
    blend_factor = weight_pos - idx_low
    lo = styled_dir / f"{frame_name}_{weights[idx_low]}.jpg"
    if not readable(lo):
        lo = None
        for w in weights:  # the first rung that exists, whether it then loads or not
            p = styled_dir / f"{frame_name}_{w}.jpg"
            if exists(p):
                lo = p if readable(p) else None
                break
    hi, w_lo, w_hi = None, 1.0, 0.0
    if lo is not None and blend_factor > 0.01 and idx_high != idx_low:
        p = styled_dir / f"{frame_name}_{weights[idx_high]}.jpg"
        if readable(p):
            hi, w_lo, w_hi = p, 1 - blend_factor, blend_factor
    return dict(orig=orig, lo=lo, hi=hi, orig_w=float(orig_blend), style_w=float(1 - orig_blend), w_lo=float(w_lo),
                w_hi=float(w_hi))


def plan(orig_dir, styled_dirs: Dict[str, str], weights: Dict[str, Sequence[str]], total_frames: int,
         readable: Callable, exists: Optional[Callable] = None, styled_start: int = 17, styled_end: int = 160,
         crossfade_frames: int = 48, hold_frames: int = 3, orig_blend: float = 0.4,
         saturation: float = 1.3) -> List[dict]:
    """The script's frame loop in Python doubles.  readable(path): the file loads (cv2.imread gives an image);
    exists(path): it is there at all (default: readable).  One entry per source frame the script writes, in order:
      {"frame": its number, "files": the distinct paths it reads, "desc": the fields of nst_multi_model_frame with
       bank indices into "files", "hold": hold_frames}
    A frame whose own original is missing has no entry.  Weights are doubles; the kernel's struct rounds each to fp32
    once."""
    exists = exists or readable
    orig_dir = Path(orig_dir)
    dirs = {k: Path(v) for k, v in styled_dirs.items()}
    if hold_frames < 1 or crossfade_frames < 0:
        raise UsageError("need --hold_frames >= 1 and a cross-fade of 0 or more frames")
    if "udnie" not in dirs:
        raise UsageError("the udnie directory is required")
    ten = weights.get("tenharmsel")
    if "tenharmsel" in dirs and ten and len(ten) <= TENHARMSEL_POS:
        raise UsageError(f"the tenharmsel ladder has {len(ten)} rungs; the compositor takes rung {TENHARMSEL_POS}")
    mosaic_weights = weights.get("mosaic", list(MOSAIC_DEFAULT))
    if "mosaic" in dirs and not mosaic_weights:
        raise UsageError("the mosaic walk file lists no weights")
    segments = [(1, styled_start - 1, None), (styled_start, styled_end, "udnie"), (styled_end + 1, total_frames, None)]
    crossfade_src_frames = crossfade_frames // hold_frames
    out = []
    for seg_idx, (start, end, style_name) in enumerate(segments):
        if start > end:
            continue
        is_last_seg = seg_idx == len(segments) - 1
        next_style = None if is_last_seg else segments[seg_idx + 1][2]
        style_weights = weights.get(style_name) if style_name else None
        for src_idx, frame_num in enumerate(range(start, end + 1)):
            frame_name = f"frame_{frame_num:04d}"
            own = orig_dir / f"{frame_name}_original.jpg"
            files: List[Path] = []

            def slot(p: Path) -> int:
                if p not in files:
                    files.append(p)
                return files.index(p)

            def still(st: dict) -> dict:
                return dict(orig=slot(st["orig"]), lo=-1 if st["lo"] is None else slot(st["lo"]),
                            hi=-1 if st["hi"] is None else slot(st["hi"]), orig_w=st["orig_w"],
                            style_w=st["style_w"], w_lo=st["w_lo"], w_hi=st["w_hi"])

            def plain(p: Path) -> dict:
                return dict(orig=slot(p), lo=-1, hi=-1, orig_w=0.0, style_w=0.0, w_lo=0.0, w_hi=0.0)

            over, keep, over_w = [], [], []
            if style_name and style_weights:
                weight_pos = ramp_position(src_idx, end - start + 1, len(style_weights))
                st = _styled_still(dirs[style_name], frame_name, style_weights, weight_pos, orig_blend, readable, exists)
                if st is None:
                    continue
                base_kind, base = _lib.NST_MM_STYLED, still(st)
                mosaic_blend, tenharmsel_blend = pulse_blends(src_idx / max(1, end - start))
                if mosaic_blend > 0.01 and "mosaic" in dirs:
                    st = _styled_still(dirs["mosaic"], frame_name, mosaic_weights, 0, orig_blend, readable, exists)
                    if st is not None:
                        over.append(still(st))
                        keep.append(float(1 - mosaic_blend))
                        over_w.append(float(mosaic_blend))
                if tenharmsel_blend > 0.01 and "tenharmsel" in dirs and ten:
                    st = _styled_still(dirs["tenharmsel"], frame_name, ten, TENHARMSEL_POS, orig_blend, readable, exists)
                    if st is not None:
                        over.append(still(st))
                        keep.append(float(1 - tenharmsel_blend))
                        over_w.append(float(tenharmsel_blend))
            else:
                if not readable(own):
                    continue
                base_kind, base = _lib.NST_MM_PLAIN, plain(own)
            desc = dict(base_kind=base_kind, base=base, n_over=len(over), over=over, keep=keep, over_w=over_w,
                        sat_on=int(bool(style_name) and saturation != 1.0), sat=float(saturation), fin=-1,
                        fin_w=(0.0, 0.0), cross_kind=_lib.NST_MM_NONE, next=None, cross_w=(0.0, 0.0))
            if style_name and src_idx < crossfade_src_frames and readable(own):
                fade_in_t = smoothstep(src_idx / crossfade_src_frames)
                desc["fin"], desc["fin_w"] = slot(own), (float(1 - fade_in_t), float(fade_in_t))
            frames_from_end = end - frame_num
            if not is_last_seg and frames_from_end < crossfade_frames:
                fade_t = smoothstep(1 - (frames_from_end / crossfade_frames))
                nxt = None
                next_weights = weights.get(next_style) if next_style else None
                if next_style is not None and next_weights:
                    st = _styled_still(dirs[next_style], frame_name, next_weights, 0, orig_blend, readable, exists)
                    if st is not None:
                        nxt = (_lib.NST_MM_STYLED, still(st))
                elif readable(own):
                    nxt = (_lib.NST_MM_PLAIN, plain(own))
                if nxt is not None:
                    desc["cross_kind"], desc["next"] = nxt
                    desc["cross_w"] = (float(1 - fade_t), float(fade_t))
            out.append(dict(frame=frame_num, files=files, desc=desc, hold=hold_frames))
    return out


def shifted(desc: dict, base: int) -> dict:
    """A plan descriptor with its bank indices moved by `base` (the frame's place in a batch's bank)."""
    def st(s):
        return None if s is None else dict(s, orig=s["orig"] + base, lo=s["lo"] + base if s["lo"] >= 0 else -1,
                                           hi=s["hi"] + base if s["hi"] >= 0 else -1)
    return dict(desc, base=st(desc["base"]), over=[st(s) for s in desc["over"]], next=st(desc["next"]),
                fin=desc["fin"] + base if desc["fin"] >= 0 else -1)


# ---- device ----
def _fill_still(a, s: dict) -> None:
    a.orig, a.lo, a.hi = int(s["orig"]), int(s["lo"]), int(s["hi"])
    a.orig_w, a.style_w, a.w_lo, a.w_hi = float(s["orig_w"]), float(s["style_w"]), float(s["w_lo"]), float(s["w_hi"])


def pack(descs: Sequence[dict]):
    """The plan's descriptors as an array of nst_multi_model_frame (doubles rounded to fp32 here, once)."""
    arr = (_lib.NstMultiModelFrame * len(descs))()
    for a, d in zip(arr, descs):
        if len(d["over"]) > 2:
            raise NstError(f"multi_model_video: a frame has at most 2 overlays, got {len(d['over'])}")
        a.base_kind, a.n_over = int(d["base_kind"]), int(d["n_over"])
        _fill_still(a.base, d["base"])
        for k, s in enumerate(d["over"]):
            _fill_still(a.over[k], s)
            a.keep[k], a.over_w[k] = float(d["keep"][k]), float(d["over_w"][k])
        a.sat_on, a.sat = int(d["sat_on"]), float(d["sat"])
        a.fin = int(d["fin"])
        a.fin_w[0], a.fin_w[1] = float(d["fin_w"][0]), float(d["fin_w"][1])
        a.cross_kind = int(d["cross_kind"])
        if d["next"] is not None:
            _fill_still(a.next, d["next"])
        a.cross_w[0], a.cross_w[1] = float(d["cross_w"][0]), float(d["cross_w"][1])
    return arr


def multi_model_frames(bank_u8: torch.Tensor, descs: Sequence[dict]) -> torch.Tensor:
    """bank uint8 [n_bank,h,w,3] on the device, descriptors as plan() emits them -> uint8 [n,h,w,3]."""
    return stills.bank_frames("multi_model_frames", "nst_multi_model_frames", pack, bank_u8, descs)


def fit_rule(size: int, portrait: bool) -> stills.FitRule:
    """The script's load_resize as stills.load_bank takes it: the whole image, scaled to fitted_size."""
    def fit(w: int, h: int):
        wh = fitted_size(w, h, size, portrait)
        if wh[0] < 1 or wh[1] < 1:
            raise NstError(f"a {w}x{h} image fits to {wh[0]}x{wh[1]}")
        return None, wh
    return fit


def load_bank(paths: Sequence, size: int = 1080, portrait: bool = True, device=None,
              jpeg_reader: str = "pil") -> torch.Tensor:
    """The script's load_resize over a list of files whose fitted sizes agree (stills.load_bank under fit_rule): uint8
    [len(paths),h,w,3] on the device; jpeg_reader "gpu" decodes the JPEGs on the device."""
    return stills.load_bank(paths, fit_rule(size, portrait), device, jpeg_reader)


def load_resize(path, size: int = 1080, portrait: bool = True, device=None) -> torch.Tensor:
    """The script's load_resize of one file: uint8 [h,w,3] on the device."""
    return load_bank([path], size, portrait, device)[0]


# ---- CLI ----
def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m neuralstyletransferv1_amd.multi_model_video",
                                 description="Pulsed multi-style video compositor over pre-styled frames on the GPU")
    ap.add_argument("--orig_dir", type=str, required=True, help="directory of frame_NNNN_original.jpg")
    ap.add_argument("--styled_udnie", type=str, required=True, help="directory of the udnie ladder stills")
    ap.add_argument("--styled_mosaic", type=str, help="directory of the mosaic stills")
    ap.add_argument("--styled_tenharmsel", type=str, help="directory of the tenharmsel ladder stills")
    ap.add_argument("--output", type=str, default=None, help="also assemble the frames with ffmpeg and write the run log")
    ap.add_argument("--styled_start", type=int, default=17, help="first styled frame")
    ap.add_argument("--styled_end", type=int, default=160, help="last styled frame")
    ap.add_argument("--total_frames", type=int, default=None, help="source frames (default: counted in --orig_dir)")
    ap.add_argument("--fps", type=int, default=24)
    ap.add_argument("--size", type=int, default=1080, help="output width")
    ap.add_argument("--portrait", action="store_true", default=True, help="always on, as in the script")
    ap.add_argument("--orig_blend", type=float, default=0.4, help="share of the original in a styled still")
    ap.add_argument("--crossfade_seconds", type=float, default=2.0)
    ap.add_argument("--hold_frames", type=int, default=3, help="output frames per source frame")
    ap.add_argument("--saturation", type=float, default=1.3, help="saturation boost of styled frames (1.0: none)")
    stills.add_output_flags(ap, "multi_model_frame")
    ap.add_argument("--jpeg_reader", choices=["pil", "gpu"], default="pil")
    ap.add_argument("--batch", type=int, default=8, help="source frames per kernel call")
    ap.add_argument("--device", type=str, default="cuda:0")
    return ap


def styled_dirs_of(args) -> Dict[str, str]:
    dirs = {"udnie": args.styled_udnie}
    if args.styled_mosaic:
        dirs["mosaic"] = args.styled_mosaic
    if args.styled_tenharmsel:
        dirs["tenharmsel"] = args.styled_tenharmsel
    return dirs


def prepare(args) -> Tuple[List[dict], Tuple[int, int]]:
    """Everything the CLI decides before it touches the device: (plan, (width, height)); UsageError for the exit-2
    cases.  Only image headers are read."""
    if args.size < 1 or args.fps < 1 or args.batch < 1 or args.hold_frames < 1 or args.crossfade_seconds < 0:
        raise UsageError("need --size, --fps, --batch, --hold_frames >= 1 and --crossfade_seconds >= 0")
    orig_dir = Path(args.orig_dir)
    dirs = styled_dirs_of(args)
    weights = load_weights(dirs)
    first = orig_dir / "frame_0001_original.jpg"
    every = sorted(orig_dir.glob("frame_*_original.jpg"))
    if not first.exists():
        if not every:
            raise UsageError(f"no frame_*_original.jpg in {orig_dir}")
        first = every[0]
    sizes: Dict[Path, Optional[Tuple[int, int]]] = {}

    def header(p: Path) -> Optional[Tuple[int, int]]:
        if p not in sizes:
            sizes[p] = header_size(p) if p.exists() else None
        return sizes[p]

    wh = header(first)
    if wh is None:
        raise UsageError(f"{first}: not a readable image")
    target = fitted_size(wh[0], wh[1], args.size, True)
    if target[1] < 1:
        raise UsageError(f"{first}: a {wh[0]}x{wh[1]} image fits to {target[0]}x{target[1]}")
    total = args.total_frames if args.total_frames is not None else len(every)
    pl = plan(orig_dir, dirs, weights, total, lambda p: header(p) is not None, lambda p: p.exists(),
              args.styled_start, args.styled_end, int(args.crossfade_seconds * args.fps), args.hold_frames,
              args.orig_blend, args.saturation)
    if not pl:
        raise UsageError(f"no frames to write: none of frames 1..{total} has its original in place")
    for fr in pl:
        for p in fr["files"]:
            got = fitted_size(*header(p), args.size, True)
            if got != target:
                raise UsageError(f"{p}: loads at {got[0]}x{got[1]}, {first} at {target[0]}x{target[1]}")
    return pl, target


def save_run_log(output_path: Path, args, styled_dirs: Dict[str, str], written: int) -> Path:
    """<stem>_run.json beside the video, with the script's keys."""
    log_path = output_path.parent / f"{output_path.stem}_run.json"
    log = {
        "timestamp": datetime.now().isoformat(),
        "script": "multi_model_video.py",
        "output_video": str(output_path),
        "duration_seconds": round(written / args.fps, 2),
        "total_frames": written,
        "parameters": {
            "orig_dir": str(args.orig_dir), "styled_start": args.styled_start, "styled_end": args.styled_end,
            "fps": args.fps, "size": args.size, "portrait": True, "orig_blend": args.orig_blend,
            "crossfade_frames": int(args.crossfade_seconds * args.fps), "hold_frames": args.hold_frames,
            "saturation": args.saturation, "smoothness": SMOOTHNESS,
        },
        "styled_dirs": {k: str(v) for k, v in styled_dirs.items()},
    }
    with open(log_path, "w") as f:
        json.dump(log, f, indent=2)
    return log_path


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = build_parser().parse_args(argv)
    try:
        pl, (tw, th) = prepare(args)
    except UsageError as e:
        print(f"[multi_model_video] {e}", file=sys.stderr)
        return 2
    device = torch.device(args.device)
    wr = stills.open_writer(args)
    print(f"[multi_model_video] {len(pl)} source frames at {tw}x{th}, {args.hold_frames} output frames each")
    for s in range(0, len(pl), args.batch):
        group = pl[s:s + args.batch]
        paths, descs = [], []
        for fr in group:  # a batch's bank: the frames' file lists one after the other
            descs.append(shifted(fr["desc"], len(paths)))
            paths += fr["files"]
        bank = load_bank(paths, args.size, True, device, args.jpeg_reader)
        frames = multi_model_frames(bank, descs)
        holds = torch.tensor([fr["hold"] for fr in group], device=device)
        wr.write(frames.repeat_interleave(holds, dim=0))
    stills.close_run("multi_model_video", wr, args.fps, args.output)
    if args.output:
        save_run_log(Path(args.output), args, styled_dirs_of(args), wr.count)
    return 0


if __name__ == "__main__":
    sys.exit(main())
