"""numpy restatement of the reference's multi-model compositor (scripts/multi_model_video.py) -- TEST
INFRASTRUCTURE ONLY.

render() keeps create_multi_model_video's frame loop (:239-353), get_styled_frame (:60-107) and adjust_saturation
(:113-122) in the script's own float32 numpy arithmetic: float32 frames, Python float scalars, the script's
expressions in the script's order, every .astype(np.uint8) where the script has one.  Files are reached through a
caller-supplied {path: u8 RGB array, or None for a file that is there but does not load}; a path that is not a key is
a missing file.  The arrays stand for load_resize's results (already fitted).  adjust_saturation's two cv2.cvtColor
calls are camera_ref.rgb_to_hsv8 / hsv8_to_rgb (cv2 is not installed: PARITY UNPINNED); frames are RGB-ordered.
evaluate() is the descriptor semantics of nst_multi_model_frames (include/nst_hip.h), written from that comment, not
from the kernel.
"""
from __future__ import annotations

import math
from pathlib import Path

import numpy as np

import camera_ref as CR

f32 = np.float32
NONE, PLAIN, STYLED = 0, 1, 2  # NST_MM_*


# ---- the script's helpers ----
def smoothstep(t):
    return t * t * (3 - 2 * t)


def gaussian_pulse(t, num_pulses=4, width=0.15):
    total = 0
    for i in range(num_pulses):
        center = (i + 0.5) / num_pulses
        total += math.exp(-((t - center) ** 2) / (2 * width ** 2))
    return min(1.0, total)


def adjust_saturation(img, factor=1.3):
    hsv = CR.rgb_to_hsv8(img).astype(np.float32)
    hsv[:, :, 1] = np.clip(hsv[:, :, 1] * factor, 0, 255)
    return CR.hsv8_to_rgb(hsv.astype(np.uint8))


def get_styled_frame(files, styled_dir, frame_name, weights, weight_pos, orig_blend=0.4):
    load = files.get
    orig = load(styled_dir / f"{frame_name}_original.jpg")
    if orig is None:
        return None
    orig = orig.astype(np.float32)
    idx_low = int(weight_pos)
    idx_high = min(idx_low + 1, len(weights) - 1)
    blend_factor = weight_pos - idx_low
    style_low = load(styled_dir / f"{frame_name}_{weights[idx_low]}.jpg")
    if style_low is None:
        for w in weights:
            p = styled_dir / f"{frame_name}_{w}.jpg"
            if p in files:
                style_low = load(p)
                break
    if style_low is None:
        return orig.astype(np.uint8)
    style_low = style_low.astype(np.float32)
    style_frame = style_low
    if blend_factor > 0.01 and idx_high != idx_low:
        style_high = load(styled_dir / f"{frame_name}_{weights[idx_high]}.jpg")
        if style_high is not None:
            style_frame = style_low * (1 - blend_factor) + style_high.astype(np.float32) * blend_factor
    frame = orig * orig_blend + style_frame * (1 - orig_blend)
    return np.clip(frame, 0, 255).astype(np.uint8)


def render(files, orig_dir, styled_dirs, weights, total_frames, styled_start=17, styled_end=160, crossfade_frames=48,
           hold_frames=3, orig_blend=0.4, saturation=1.3):
    """files: {Path: u8 [h,w,3] or None}; styled_dirs {'udnie': dir, ['mosaic': dir], ['tenharmsel': dir]}; weights
    {style: the walk file's `weights`} for the styles that have a walk file.  Returns the u8 frames the script hands
    to its writer, hold copies included."""
    orig_dir = Path(orig_dir)
    styled_dirs = {k: Path(v) for k, v in styled_dirs.items()}
    load = files.get
    segments = [(1, styled_start - 1, None), (styled_start, styled_end, "udnie"), (styled_end + 1, total_frames, None)]
    written = []
    for seg_idx, (start, end, style_name) in enumerate(segments):
        if start > end:
            continue
        is_last_seg = seg_idx == len(segments) - 1
        next_seg = None if is_last_seg else segments[seg_idx + 1]
        style_dir = styled_dirs.get(style_name, orig_dir) if style_name else orig_dir
        style_weights = weights.get(style_name, None)
        for src_idx, frame_num in enumerate(range(start, end + 1)):
            frame_name = f"frame_{frame_num:04d}"
            if style_name and style_weights:
                segment_frames = end - start + 1
                usable_weights = len(style_weights)
                frames_per_weight = max(1, segment_frames // usable_weights)
                weight_idx = min(src_idx // frames_per_weight, usable_weights - 1)
                weight_progress = (src_idx % frames_per_weight) / frames_per_weight
                weight_pos = 0 + weight_idx + weight_progress * 0.5
                frame = get_styled_frame(files, style_dir, frame_name, style_weights, weight_pos, orig_blend)
                if style_name == "udnie":
                    segment_progress = src_idx / max(1, (end - start))
                    frame_f = frame.astype(np.float32) if frame is not None else None
                    mosaic_blend = gaussian_pulse(segment_progress, num_pulses=4, width=0.10) * 0.5
                    tenharmsel_blend = gaussian_pulse(segment_progress + 0.125, num_pulses=4, width=0.10) * 0.5
                    if mosaic_blend > 0.01 and "mosaic" in styled_dirs and frame_f is not None:
                        mosaic_weights = weights.get("mosaic", ["mosaic_style5e10"])
                        mosaic_frame = get_styled_frame(files, styled_dirs["mosaic"], frame_name, mosaic_weights, 0,
                                                        orig_blend)
                        if mosaic_frame is not None:
                            frame_f = frame_f * (1 - mosaic_blend) + mosaic_frame.astype(np.float32) * mosaic_blend
                    if tenharmsel_blend > 0.01 and "tenharmsel" in styled_dirs and frame_f is not None:
                        tenharmsel_weights = weights.get("tenharmsel", None)
                        if tenharmsel_weights:
                            tenharmsel_frame = get_styled_frame(files, styled_dirs["tenharmsel"], frame_name,
                                                                tenharmsel_weights, 5, orig_blend)
                            if tenharmsel_frame is not None:
                                frame_f = (frame_f * (1 - tenharmsel_blend)
                                           + tenharmsel_frame.astype(np.float32) * tenharmsel_blend)
                    if frame_f is not None:
                        frame = np.clip(frame_f, 0, 255).astype(np.uint8)
            else:
                frame = load(orig_dir / f"{frame_name}_original.jpg")
            if frame is None:
                continue
            frame = frame.astype(np.float32)
            if style_name and saturation != 1.0:
                frame = adjust_saturation(np.clip(frame, 0, 255).astype(np.uint8), saturation).astype(np.float32)
            crossfade_src_frames = crossfade_frames // hold_frames
            if style_name and src_idx < crossfade_src_frames:
                fade_in_t = smoothstep(src_idx / crossfade_src_frames)
                orig_frame = load(orig_dir / f"{frame_name}_original.jpg")
                if orig_frame is not None:
                    frame = orig_frame.astype(np.float32) * (1 - fade_in_t) + frame * fade_in_t
            frames_from_end = end - frame_num
            if not is_last_seg and frames_from_end < crossfade_frames:
                fade_t = smoothstep(1 - (frames_from_end / crossfade_frames))
                next_style = next_seg[2]
                next_weights = weights.get(next_style, None) if next_style is not None else None
                if next_style is not None and next_weights:
                    next_frame = get_styled_frame(files, styled_dirs.get(next_style, orig_dir), frame_name,
                                                  next_weights, 0, orig_blend)
                else:
                    next_frame = load(orig_dir / f"{frame_name}_original.jpg")
                if next_frame is not None:
                    frame = frame * (1 - fade_t) + next_frame.astype(np.float32) * fade_t
            assert frame.dtype == np.float32
            frame = np.clip(frame, 0, 255).astype(np.uint8)
            written += [frame] * hold_frames
    return written


# ---- the descriptor semantics of nst_multi_model_frames ----
def trunc(x):
    return np.clip(x, 0, 255).astype(np.uint8)


def still(bank, s, styled=True):
    """ST(s), or the plain image s["orig"]."""
    if not styled or s["lo"] < 0:
        return bank[s["orig"]]
    lo = bank[s["lo"]].astype(f32)
    sf = lo if s["hi"] < 0 else lo * f32(s["w_lo"]) + bank[s["hi"]].astype(f32) * f32(s["w_hi"])
    return trunc(bank[s["orig"]].astype(f32) * f32(s["orig_w"]) + sf * f32(s["style_w"]))


def saturate(px, factor):
    hsv = CR.rgb_to_hsv8(px)
    hsv[..., 1] = trunc(hsv[..., 1].astype(f32) * f32(factor))
    return CR.hsv8_to_rgb(hsv.astype(np.uint8))


def evaluate(bank, d):
    """One frame from its descriptor (the dict multi_model_video.plan emits; every weight rounded to fp32 once)."""
    F = still(bank, d["base"], d["base_kind"] == STYLED).astype(f32)
    for k in range(d["n_over"]):
        F = F * f32(d["keep"][k]) + still(bank, d["over"][k]).astype(f32) * f32(d["over_w"][k])
    U = trunc(F)
    if d["sat_on"]:
        U = saturate(U, d["sat"])
    G = U.astype(f32)
    if d["fin"] >= 0:
        G = bank[d["fin"]].astype(f32) * f32(d["fin_w"][0]) + G * f32(d["fin_w"][1])
    if d["cross_kind"] != NONE:
        N = still(bank, d["next"], d["cross_kind"] == STYLED)
        G = G * f32(d["cross_w"][0]) + N.astype(f32) * f32(d["cross_w"][1])
    assert G.dtype == f32
    return trunc(G)


# ---- the layout the host and the CLI tests share ----
# 12 source frames, styled 4..9, at --fps 3 --crossfade_seconds 2.0 (6 cross-fade frames) --hold_frames 2 (a 3-frame
# fade-in): an udnie ladder of 3 rungs (walk_udnie.json), mosaic without a walk file (the script's one default rung),
# a tenharmsel ladder of 6 rungs (walk.json) of which only rung 5 is ever read.  Every styled directory holds a copy of
# the originals it blends with.  What is left out, and why:
#   orig     frame 11                    a skipped frame (no hold copies)
#   udnie    frames 1..3 have no rungs   the intro cross-fades into the lo < 0 fallback, the copy of the original
#            frame 7 rung 2              a missing high rung (position 1.25): the low rung alone
#            frame 8 rung 2              a missing low rung (position 2): the first rung that exists
#   mosaic   originals 5, 6              a missing overlay original: tenharmsel alone on 5
#   tenharmsel original 6                no overlay at all on 6
#            frame 9 rung 5 unreadable   (None) the overlay is its copy of the original
UDNIE = ("udnie_style5e10", "udnie_style1e11", "udnie_style5e11")
TENHARMSEL = tuple(f"tenharmsel_style{v}" for v in ("1e9", "5e9", "1e10", "5e10", "1e11", "5e11"))
LAYOUT = dict(
    total_frames=12, styled_start=4, styled_end=9, fps=3, crossfade_seconds=2.0, hold_frames=2,
    weights={"udnie": UDNIE, "tenharmsel": TENHARMSEL},
    walk_names={"udnie": "walk_udnie.json", "tenharmsel": "walk.json"},
)


def layout_files():
    """[(directory key, file name, kind)]: kind "orig" (a copy of that frame's original), "rung" (an image of its own)
    or "bad" (there, but does not load)."""
    out = [("orig", f"frame_{n:04d}_original.jpg", "orig") for n in range(1, 13) if n != 11]
    out += [("udnie", f"frame_{n:04d}_original.jpg", "orig") for n in range(1, 10)]
    for n in range(4, 10):
        for r, wt in enumerate(UDNIE):
            if not (r == 2 and n in (7, 8)):
                out.append(("udnie", f"frame_{n:04d}_{wt}.jpg", "rung"))
        out.append(("mosaic", f"frame_{n:04d}_mosaic_style5e10.jpg", "rung"))
        out.append(("tenharmsel", f"frame_{n:04d}_{TENHARMSEL[5]}.jpg", "bad" if n == 9 else "rung"))
        if n not in (5, 6):
            out.append(("mosaic", f"frame_{n:04d}_original.jpg", "orig"))
        if n != 6:
            out.append(("tenharmsel", f"frame_{n:04d}_original.jpg", "orig"))
    return out


def layout_dirs(root):
    return {k: Path(root) / k for k in ("orig", "udnie", "mosaic", "tenharmsel")}


def write_layout(root, orig_wh=(64, 50), rung_wh=(48, 37), seed=200):
    """LAYOUT as Pillow JPEGs under root/orig, root/udnie, ...: every copy of an original the same file, rungs images
    of their own, the "bad" file junk bytes, and the two walk files.  Returns layout_dirs(root)."""
    import json

    from PIL import Image
    dirs = layout_dirs(root)
    for d in dirs.values():
        d.mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(seed)

    def jpeg(wh):
        # smooth content (a random 6x6 grid enlarged) so that the JPEG is an ordinary photograph-like file
        import io
        small = rng.integers(0, 256, (6, 6, 3), dtype=np.uint8)
        buf = io.BytesIO()
        Image.fromarray(small).resize(wh, Image.BICUBIC).save(buf, format="JPEG", quality=92)
        return buf.getvalue()

    originals = {}
    for key, name, kind in layout_files():
        if kind == "orig":
            if name not in originals:
                originals[name] = jpeg(orig_wh)
            data = originals[name]
        else:
            data = jpeg(rung_wh) if kind == "rung" else b"not a jpeg"
        (dirs[key] / name).write_bytes(data)
    for style, name in LAYOUT["walk_names"].items():
        wts = list(LAYOUT["weights"][style])
        (dirs[style] / name).write_text(json.dumps({"walk": [0.5] * 4, "weights": wts}))
    return dirs


def layout_arrays(dirs, h, w, seed=9):
    """render()'s `files` for LAYOUT with random u8 images; dirs {"orig" / "udnie" / "mosaic" / "tenharmsel": path}."""
    rng = np.random.default_rng(seed)
    originals, files = {}, {}
    for key, name, kind in layout_files():
        if kind == "bad":
            img = None
        elif kind == "orig":
            if name not in originals:
                originals[name] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            img = originals[name]
        else:
            img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        files[Path(dirs[key]) / name] = img
    return files
