"""Style morph on the MI355X engine: the reference's cross-image weight flow (scripts/style_morph.py) over the
ladder stills the stylizer writes (`NAME_candy.jpg`, `NAME_candy_style1e9.jpg`, ... `NAME_tenharmsel_style1e12.jpg`
beside `NAME_original.jpg`).

Every still drifts along each family's weight ladder with slow sine waves of the global time, blends up to five
families plus the original, cross-fades into the next still over int(fps * 1.5) frames and gets one gentle colour
filter.  The reference loops over float32 numpy frames; here

  plan()                  the script's scalars, in double, per output frame -> descriptors + the images each still needs
  style_morph_frames()    nst_style_morph_frames: blend, clip, truncate and filter in one pass over the u8 stills

The blend is the reference's own numpy float32 arithmetic (each Python scalar rounded to fp32 once, every product and
sum on its own), so frames equal the script's byte for byte given the same stills.  What is restated, parity unpinned
(cv2 is not installed here): cv2.imread is Pillow's decode, the fit is camera.lanczos_resize (INTER_LANCZOS4), and
the filters' two cvtColor calls are the camera stage's 8-bit HSV conversions.  tests/style_morph_ref.py is the numpy
yardstick.

The script draws an unseeded random.choice(FILTERS) per image; here --filter fixes it or --seed (default 0) seeds
random.Random(seed).choice, drawn once per loaded image in order.

Out of scope (not built): cv2's VideoWriter and the H.264 re-encode (assemble_video replaces them), the Magenta back
end, face detection.  The stills' other consumer, multi_model_video.py, is its own module (multi_model_video.py here).
"""
from __future__ import annotations

import argparse
import math
import random
import sys
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib, stills as shared  # `stills` names the collected images in this module
from ._lib import NstError
from .stills import UsageError, header_size

_WEIGHTS = ("1e9", "5e9", "1e10", "5e10", "1e11", "5e11", "1e12")
_TENHARMSEL = tuple(f"{m}e{e}" for e in (9, 10, 11) for m in range(1, 10)) + ("1e12",)
# the script's weight ladders, ordered low to high: four families of 8 rungs, tenharmsel of 28
LADDERS: Dict[str, Tuple[str, ...]] = {
    "candy": ("candy",) + tuple(f"candy_style{v}" for v in _WEIGHTS),
    "udnie": ("udnie",) + tuple(f"udnie_style{v}" for v in _WEIGHTS),
    "mosaic": ("mosaic",) + tuple(f"mosaic_style{v}" for v in _WEIGHTS),
    "rain_princess": ("rain_princess",) + tuple(f"rain_princess_style{v}" for v in _WEIGHTS),
    "tenharmsel": tuple(f"tenharmsel_style{v}" for v in _TENHARMSEL),
}
FILTERS = ("none", "subtle_sat", "vibrance", "warm")
# FILTERS' parameters as the kernel takes them, each evaluated in double (the kernel's struct rounds them to fp32
# once): boost_saturation(x, 1.08); vibrance(x, 1.08): factor, 1 - factor; warm_filter(x, 0.05) on R, G, B (the
# script's BGR channels 2, 1, 0)
FILTER_PARAMS = {
    "none": (_lib.NST_SM_FILTER_NONE, (0.0, 0.0, 0.0)),
    "subtle_sat": (_lib.NST_SM_FILTER_SAT, (1.08, 0.0, 0.0)),
    "vibrance": (_lib.NST_SM_FILTER_VIBRANCE, (1.08, 1 - 1.08, 0.0)),
    "warm": (_lib.NST_SM_FILTER_WARM, (1 + 0.05, 1 + 0.05 * 0.3, 1 - 0.05 * 0.3)),
}
ORIGINAL = ("original", 0)  # a still's key of its unstyled image; a ladder image's key is (family, rung)


# ---- discovery ----
def discover(styled_dir, skip_first: bool = True) -> List[str]:
    """The script's image names: stem.rsplit('_', 1)[0] over *.jpg with a '_' in the stem, sorted; the first one
    removed when skip_first (and more than one).  The rule also yields names such as IMG_001_candy (from
    IMG_001_candy_style1e9.jpg); those have no _original.jpg and drop out in collect()."""
    names = sorted(set(f.stem.rsplit("_", 1)[0] for f in Path(styled_dir).glob("*.jpg") if "_" in f.stem))
    if skip_first and len(names) > 1:
        names = names[1:]
    return names


def select_ladders(families: Optional[Sequence[str]]) -> Dict[str, Tuple[str, ...]]:
    """--families: the script's filter over its ladder table (table order kept); an unknown name is an error."""
    if not families:
        return dict(LADDERS)
    unknown = [f for f in families if f not in LADDERS]
    if unknown:
        raise UsageError(f"unknown style family {', '.join(unknown)} (known: {', '.join(LADDERS)})")
    return {k: v for k, v in LADDERS.items() if k in families}


def fitted_size(w: int, h: int, size: int, portrait: bool) -> Tuple[int, int]:
    """(width, height) load_resize gives a w x h source."""
    return (int(w * (size / h)), size) if portrait else (size, size)


def collect(styled_dir, names: Sequence[str], ladders: Dict[str, Tuple[str, ...]], size: int = 1080,
            portrait: bool = False, filter_name: str = "random", seed: int = 0) -> List[dict]:
    """The script's preload loop without the pixels: per usable name (an _original.jpg and at least one ladder image)
    {"name", "orig": path, "ladders": {family: [paths of the rungs that exist]}, "filter", "sizes": {path: fitted
    (w, h)}}.  Only image headers are read."""
    if filter_name != "random" and filter_name not in FILTERS:
        raise UsageError(f"unknown filter {filter_name!r}")
    rng = random.Random(seed)
    root = Path(styled_dir)
    stills = []
    for name in names:
        sizes = {}

        def present(style: str) -> Optional[Path]:
            p = root / f"{name}_{style}.jpg"
            wh = header_size(p) if p.exists() else None
            if wh is None:
                return None
            sizes[p] = fitted_size(wh[0], wh[1], size, portrait)
            return p

        orig = present("original")
        if orig is None:
            continue
        found = {}
        for fam, ladder in ladders.items():
            paths = [p for p in (present(s) for s in ladder) if p is not None]
            if paths:
                found[fam] = paths
        if not found:
            continue
        flt = rng.choice(FILTERS) if filter_name == "random" else filter_name
        stills.append(dict(name=name, orig=orig, ladders=found, filter=flt, sizes=sizes))
    return stills


# ---- the plan ----
def get_ladder_position(style_idx: int, global_t: float) -> float:
    freq = 0.3 + style_idx * 0.15
    phase = style_idx * 0.25
    return 0.5 + 0.5 * math.sin((global_t * freq + phase) * math.pi * 2)


def get_style_weight(style_idx: int, global_t: float) -> float:
    freq = 0.2 + style_idx * 0.1
    phase = style_idx * 0.3
    raw = 0.5 + 0.5 * math.sin((global_t * freq + phase) * math.pi * 2)
    return max(0.1, raw)


def frame_counts(frame_time: float, fps: int) -> Tuple[int, int]:
    """(frame_count, crossfade_frames) = (int(fps * frame_time), int(fps * 1.5))."""
    return int(fps * frame_time), int(fps * 1.5)


def total_frames(n_images: int, frame_count: int, crossfade_frames: int) -> int:
    return frame_count + (n_images - 1) * (frame_count - crossfade_frames)


def _side(families: Sequence[Tuple[str, int]], global_t: float, orig_blend: float) -> dict:
    """One still's blend at a global time: the original's weight and per available family the two rungs, their
    smoothstep weights and the normalised family weight.  style_idx counts this still's available families."""
    terms, raw = [], []
    for style_idx, (fam, rungs) in enumerate(families):
        position = get_ladder_position(style_idx, global_t)
        if rungs == 1:
            lo, hi, w_lo, w_hi = 0, -1, 1.0, 0.0
        else:
            idx_float = position * (rungs - 1)
            lo = int(idx_float)
            hi = min(lo + 1, rungs - 1)
            blend = idx_float - lo
            blend = blend * blend * (3 - 2 * blend)
            w_lo, w_hi = 1 - blend, blend
        terms.append(dict(lo=(fam, lo), hi=None if hi < 0 else (fam, hi), w_lo=float(w_lo), w_hi=float(w_hi)))
        raw.append(get_style_weight(style_idx, global_t))
    total_weight = sum(raw)
    style_total = 1.0 - orig_blend
    for t, w in zip(terms, raw):
        t["weight"] = float(style_total * w / total_weight)
    return dict(orig_w=float(orig_blend), terms=terms)


def plan(images: Sequence[dict], frame_time: float = 4.0, fps: int = 24, orig_blend: float = 0.08) -> dict:
    """The script's frame loop in Python doubles.  images[i] = {"families": [(family, rungs), ...] in the still's own
    order, "filter": one of FILTERS}.  Returns {"frames": [...], "needs": [...]}:
      needs[i]   the images still i's frames read, as keys ORIGINAL / (family, rung), in bank order
      frames[k]  {"still": i, "n_sides", "fade": (f0, f1), "sides": [{"orig", "orig_w", "terms": [{"lo", "hi", "w_lo",
                 "w_hi", "weight"}]}], "filter", "fparam"}: the fields of nst_style_morph_frame; the bank of a frame
                 of still i is needs[i] followed by needs[i + 1], "hi" is -1 for a one-rung ladder.
    Weights are doubles; the kernel's struct rounds each to fp32 once."""
    k = len(images)
    frame_count, crossfade_frames = frame_counts(frame_time, fps)
    if k < 2:
        raise UsageError(f"need at least 2 usable images, got {k}")
    if frame_count < crossfade_frames:
        raise UsageError(f"int(fps * frame_time) = {frame_count} frames per image is shorter than the cross-fade's "
                         f"int(fps * 1.5) = {crossfade_frames}")
    for im in images:
        if not 1 <= len(im["families"]) <= _lib.NST_STYLE_MORPH_MAX_STYLES or im["filter"] not in FILTERS:
            raise UsageError(f"an image takes 1..{_lib.NST_STYLE_MORPH_MAX_STYLES} families and a filter of {FILTERS}")
    total_video_frames = k * frame_count
    raw_frames = []
    used: List[Dict[Tuple[str, int], None]] = [{ORIGINAL: None} for _ in range(k)]  # insertion-ordered sets
    for idx, im in enumerate(images):
        is_last = idx == k - 1
        for f in range(frame_count):
            if idx > 0 and f < crossfade_frames:
                continue  # shown inside the previous image's cross-fade
            global_t = (idx * frame_count + f) / total_video_frames
            sides = [(idx, _side(im["families"], global_t, orig_blend))]
            fade = (1.0, 0.0)
            if not is_last and f >= frame_count - crossfade_frames:
                fade_progress = (f - (frame_count - crossfade_frames)) / crossfade_frames
                fade_t = fade_progress * fade_progress * (3 - 2 * fade_progress)
                next_global_frame = (idx + 1) * frame_count + int(fade_progress * crossfade_frames * 0.3)
                next_global_t = next_global_frame / total_video_frames
                sides.append((idx + 1, _side(images[idx + 1]["families"], next_global_t, orig_blend)))
                fade = (float(1 - fade_t), float(fade_t))
            for still, sd in sides:
                for t in sd["terms"]:
                    used[still][t["lo"]] = None
                    if t["hi"] is not None:
                        used[still][t["hi"]] = None
            raw_frames.append((idx, sides, fade))
    needs = [sorted(u, key=lambda key: (key != ORIGINAL, key)) for u in used]
    slot = [{key: i for i, key in enumerate(n)} for n in needs]
    frames = []
    for idx, sides, fade in raw_frames:
        out_sides = []
        for still, sd in sides:
            base = 0 if still == idx else len(needs[idx])
            terms = [dict(lo=base + slot[still][t["lo"]], hi=-1 if t["hi"] is None else base + slot[still][t["hi"]],
                          w_lo=t["w_lo"], w_hi=t["w_hi"], weight=t["weight"]) for t in sd["terms"]]
            out_sides.append(dict(orig=base + slot[still][ORIGINAL], orig_w=sd["orig_w"], terms=terms))
        code, fparam = FILTER_PARAMS[images[idx]["filter"]]
        frames.append(dict(still=idx, n_sides=len(out_sides), fade=fade, sides=out_sides, filter=code, fparam=fparam))
    assert len(frames) == total_frames(k, frame_count, crossfade_frames)
    return dict(frames=frames, needs=needs)


# ---- device ----
def pack(descs: Sequence[dict]):
    """The plan's descriptors as an array of nst_style_morph_frame (doubles rounded to fp32 here, once)."""
    arr = (_lib.NstStyleMorphFrame * len(descs))()
    for a, d in zip(arr, descs):
        a.n_sides = int(d["n_sides"])
        a.fade[0], a.fade[1] = float(d["fade"][0]), float(d["fade"][1])
        a.filter = int(d["filter"])
        for j in range(3):
            a.fparam[j] = float(d["fparam"][j])
        if len(d["sides"]) > 2:
            raise NstError(f"style_morph: a frame has at most 2 sides, got {len(d['sides'])}")
        for s, sd in zip(a.side, d["sides"]):
            if len(sd["terms"]) > _lib.NST_STYLE_MORPH_MAX_STYLES:
                raise NstError(f"style_morph: at most {_lib.NST_STYLE_MORPH_MAX_STYLES} terms per side")
            s.orig, s.orig_w, s.n_terms = int(sd["orig"]), float(sd["orig_w"]), len(sd["terms"])
            for t, td in zip(s.term, sd["terms"]):
                t.lo, t.hi = int(td["lo"]), int(td["hi"])
                t.w_lo, t.w_hi, t.weight = float(td["w_lo"]), float(td["w_hi"]), float(td["weight"])
    return arr


def style_morph_frames(bank_u8: torch.Tensor, descs: Sequence[dict]) -> torch.Tensor:
    """bank uint8 [n_bank,h,w,3] on the device, descriptors as plan() emits them -> uint8 [n,h,w,3]."""
    return shared.bank_frames("style_morph_frames", "nst_style_morph_frames", pack, bank_u8, descs)


def fit_rule(size: int, portrait: bool) -> shared.FitRule:
    """The script's load_resize as stills.load_bank takes it: the square centre crop or, portrait, the whole image at
    height `size`."""
    def fit(w: int, h: int):
        tw, th = fitted_size(w, h, size, portrait)
        if tw < 1:
            raise NstError(f"portrait width int({w} * {size} / {h}) is 0")
        side = min(w, h)
        return (None if portrait else ((w - side) // 2, (h - side) // 2, side, side)), (tw, th)
    return fit


def load_resize(path, size: int = 1080, portrait: bool = False, device=None) -> torch.Tensor:
    """The script's load_resize of one file (stills.load_bank under fit_rule): uint8 [h,w,3] on the device."""
    return shared.load_bank([path], fit_rule(size, portrait), device)[0]


def still_images(still: dict) -> Dict[Tuple[str, int], Path]:
    """key -> path of every image collect() found for a still."""
    keys = {ORIGINAL: still["orig"]}
    for fam, paths in still["ladders"].items():
        for rung, p in enumerate(paths):
            keys[(fam, rung)] = p
    return keys


def load_bank(still: dict, needs: Sequence[Tuple[str, int]], size: int, portrait: bool, device) -> torch.Tensor:
    """The images of `needs`, in that order: uint8 [len(needs),h,w,3] on the device."""
    paths = still_images(still)
    return shared.load_bank([paths[key] for key in needs], fit_rule(size, portrait), device)


# ---- CLI ----
def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m neuralstyletransferv1_amd.style_morph",
                                 description="Weight-ladder style flow across pre-styled stills on the GPU")
    ap.add_argument("--styled_dir", type=str, required=True, help="directory of NAME_original.jpg and NAME_<style>.jpg")
    ap.add_argument("--frame_time", type=float, default=4.0, help="seconds per image")
    ap.add_argument("--size", type=int, default=1080)
    ap.add_argument("--fps", type=int, default=24)
    ap.add_argument("--no_skip_first", action="store_true")
    ap.add_argument("--portrait", action="store_true", help="keep the aspect ratio, scale to height --size")
    ap.add_argument("--orig_blend", type=float, default=0.08, help="share of the original image (0-1)")
    ap.add_argument("--families", type=str, nargs="+", help=f"style families to use (of {', '.join(LADDERS)})")
    ap.add_argument("--filter", choices=("random",) + FILTERS, default="random", help="every image's colour filter")
    ap.add_argument("--seed", type=int, default=0, help="seed of --filter random")
    shared.add_output_flags(ap, "style_morph_frame")
    ap.add_argument("--output_video", "--output", dest="output_video", type=str, default=None,
                    help="also assemble the frames with ffmpeg")
    ap.add_argument("--batch", type=int, default=24, help="frames per kernel call (and per write)")
    ap.add_argument("--device", type=str, default="cuda:0")
    return ap


def prepare(args) -> Tuple[List[dict], dict]:
    """Everything the CLI decides before it touches the device: (stills, plan); UsageError for the exit-2 cases."""
    if args.size < 1 or args.fps < 1 or args.batch < 1 or not args.frame_time > 0 or not 0.0 <= args.orig_blend < 1.0:
        raise UsageError("need --size, --fps, --batch >= 1, --frame_time > 0 and 0 <= --orig_blend < 1")
    ladders = select_ladders(args.families)
    names = discover(args.styled_dir, not args.no_skip_first)
    stills = collect(args.styled_dir, names, ladders, args.size, args.portrait, args.filter, args.seed)
    if len(stills) < 2:
        raise UsageError(f"need at least 2 usable images (an _original.jpg and one ladder image each), got {len(stills)}")
    first = next(iter(stills[0]["sizes"].values()))
    for st in stills:
        for p, wh in st["sizes"].items():
            if wh != first:
                raise UsageError(f"{p}: loads at {wh[0]}x{wh[1]}, {stills[0]['orig']} at {first[0]}x{first[1]}")
    images = [dict(families=[(fam, len(paths)) for fam, paths in st["ladders"].items()], filter=st["filter"])
              for st in stills]
    return stills, plan(images, args.frame_time, args.fps, args.orig_blend)


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = build_parser().parse_args(argv)
    try:
        stills, pl = prepare(args)
    except UsageError as e:
        print(f"[style_morph] {e}", file=sys.stderr)
        return 2
    device = torch.device(args.device)
    wr = shared.open_writer(args)
    frames, needs = pl["frames"], pl["needs"]
    cur = load_bank(stills[0], needs[0], args.size, args.portrait, device)
    pos = 0
    for idx, st in enumerate(stills):
        # the banks of this still and the next stay on the device: a cross-fade frame reads both
        nxt = load_bank(stills[idx + 1], needs[idx + 1], args.size, args.portrait, device) if idx + 1 < len(stills) else None
        bank = cur if nxt is None else torch.cat([cur, nxt])
        end = pos
        while end < len(frames) and frames[end]["still"] == idx:
            end += 1
        for s in range(pos, end, args.batch):
            wr.write(style_morph_frames(bank, frames[s:min(end, s + args.batch)]))
        pos = end
        cur = nxt
        print(f"[style_morph] {idx + 1}/{len(stills)} {st['name']} ({st['filter']}): {wr.count} frames")
    assert pos == len(frames) == wr.count
    shared.close_run("style_morph", wr, args.fps, args.output_video)
    return 0


if __name__ == "__main__":
    sys.exit(main())
