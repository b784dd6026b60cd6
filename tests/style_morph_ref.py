"""numpy restatement of the reference's style morph (scripts/style_morph.py) -- TEST INFRASTRUCTURE ONLY.

render() keeps create_video's frame loop (:216-298) and interpolate_ladder (:105-118) literally: float32 frames,
Python float scalars, the script's expressions in the script's order, so the blend IS the reference's numpy
arithmetic.  The three filters (:42-59) keep their numpy lines; their two cv2.cvtColor calls are
camera_ref.rgb_to_hsv8 / hsv8_to_rgb (cv2 is not installed: PARITY UNPINNED), and frames are RGB-ordered, so the warm
filter's BGR channels 2, 1, 0 are 0, 1, 2 here.  evaluate() is the descriptor semantics of nst_style_morph_frames
(include/nst_hip.h), written from that comment, not from the kernel.
"""
from __future__ import annotations

import math

import numpy as np

import camera_ref as CR

f32 = np.float32


# ---- the filters ----
def boost_saturation(img, factor=1.10):
    hsv = CR.rgb_to_hsv8(img).astype(np.float32)
    hsv[:, :, 1] = np.clip(hsv[:, :, 1] * factor, 0, 255)
    return CR.hsv8_to_rgb(hsv.astype(np.uint8))


def warm_filter(img, strength=0.06):
    img = img.astype(np.float32)
    img[:, :, 0] = np.clip(img[:, :, 0] * (1 + strength), 0, 255)
    img[:, :, 1] = np.clip(img[:, :, 1] * (1 + strength * 0.3), 0, 255)
    img[:, :, 2] = np.clip(img[:, :, 2] * (1 - strength * 0.3), 0, 255)
    return img.astype(np.uint8)


def vibrance(img, factor=1.10):
    hsv = CR.rgb_to_hsv8(img).astype(np.float32)
    sat = hsv[:, :, 1]
    boost = factor + (1 - factor) * (sat / 255)
    hsv[:, :, 1] = np.clip(sat * boost, 0, 255)
    return CR.hsv8_to_rgb(hsv.astype(np.uint8))


FILTERS = {
    "none": lambda x: x,
    "subtle_sat": lambda x: boost_saturation(x, 1.08),
    "vibrance": lambda x: vibrance(x, 1.08),
    "warm": lambda x: warm_filter(x, 0.05),
}


def interpolate_ladder(images, position):
    if len(images) == 1:
        return images[0]
    idx_float = position * (len(images) - 1)
    idx_low = int(idx_float)
    idx_high = min(idx_low + 1, len(images) - 1)
    blend = idx_float - idx_low
    blend = blend * blend * (3 - 2 * blend)
    return images[idx_low] * (1 - blend) + images[idx_high] * blend


def get_ladder_position(style_idx, global_t):
    freq = 0.3 + style_idx * 0.15
    phase = style_idx * 0.25
    return 0.5 + 0.5 * math.sin((global_t * freq + phase) * math.pi * 2)


def get_style_weight(style_idx, global_t, num_active):
    freq = 0.2 + style_idx * 0.1
    phase = style_idx * 0.3
    raw = 0.5 + 0.5 * math.sin((global_t * freq + phase) * math.pi * 2)
    return max(0.1, raw)


def render(image_data, frame_time=4.0, fps=24, orig_blend=0.08):
    """image_data[i] = {"orig": u8 [h,w,3], "ladders": {family: [u8 images]} (insertion-ordered), "filter": name}.
    Returns the list of u8 frames the script hands to its writer."""
    image_data = [dict(orig=d["orig"].astype(np.float32),
                       ladders={k: [im.astype(np.float32) for im in v] for k, v in d["ladders"].items()},
                       filter_fn=FILTERS[d["filter"]]) for d in image_data]
    num_images = len(image_data)
    frame_count = int(fps * frame_time)
    crossfade_frames = int(fps * 1.5)
    total_video_frames = num_images * frame_count
    written = []
    for idx, data in enumerate(image_data):
        is_first = (idx == 0)
        is_last = (idx == len(image_data) - 1)
        next_data = image_data[idx + 1] if not is_last else None
        available_styles = list(data["ladders"].keys())
        for f in range(frame_count):
            global_frame = idx * frame_count + f
            global_t = global_frame / total_video_frames
            ORIG_AMOUNT = orig_blend
            STYLE_TOTAL = 1.0 - orig_blend
            style_contributions = []
            for style_idx, style_name in enumerate(available_styles):
                ladder_imgs = data["ladders"][style_name]
                ladder_pos = get_ladder_position(style_idx, global_t)
                style_frame = interpolate_ladder(ladder_imgs, ladder_pos)
                weight = get_style_weight(style_idx, global_t, len(available_styles))
                style_contributions.append((style_frame, weight))
            total_weight = sum(w for _, w in style_contributions)
            style_contributions = [(fr, STYLE_TOTAL * w / total_weight) for fr, w in style_contributions]
            frame = data["orig"] * ORIG_AMOUNT
            for style_frame, weight in style_contributions:
                if style_frame is not None:
                    frame += style_frame * weight
            if not is_last and f >= frame_count - crossfade_frames:
                fade_progress = (f - (frame_count - crossfade_frames)) / crossfade_frames
                fade_t = fade_progress * fade_progress * (3 - 2 * fade_progress)
                next_global_frame = (idx + 1) * frame_count + int(fade_progress * crossfade_frames * 0.3)
                next_global_t = next_global_frame / total_video_frames
                next_available = list(next_data["ladders"].keys())
                next_contributions = []
                for style_idx, style_name in enumerate(next_available):
                    ladder_imgs = next_data["ladders"][style_name]
                    ladder_pos = get_ladder_position(style_idx, next_global_t)
                    style_frame = interpolate_ladder(ladder_imgs, ladder_pos)
                    weight = get_style_weight(style_idx, next_global_t, len(next_available))
                    next_contributions.append((style_frame, weight))
                next_total = sum(w for _, w in next_contributions)
                next_contributions = [(fr, STYLE_TOTAL * w / next_total) for fr, w in next_contributions]
                next_frame = next_data["orig"] * ORIG_AMOUNT
                for style_frame, weight in next_contributions:
                    if style_frame is not None:
                        next_frame += style_frame * weight
                frame = frame * (1 - fade_t) + next_frame * fade_t
            if not is_first and f < crossfade_frames:
                continue
            assert frame.dtype == np.float32
            frame = np.clip(frame, 0, 255).astype(np.uint8)
            written.append(data["filter_fn"](frame))
    return written


# ---- the descriptor semantics of nst_style_morph_frames ----
def apply_filter(px, code, fparam):
    """The kernel's filter step on a u8 image: code 0 none, 1 saturation, 2 vibrance, 3 warm; fparam three floats."""
    p = [f32(v) for v in fparam]
    if code == 0:
        return px
    if code == 3:
        return np.clip(px.astype(f32) * np.array(p, f32), 0, 255).astype(np.uint8)
    hsv = CR.rgb_to_hsv8(px)
    s = hsv[..., 1].astype(f32)
    boost = p[0] if code == 1 else p[0] + p[1] * (s / f32(255))
    hsv[..., 1] = np.clip(s * boost, 0, 255).astype(np.uint8)
    return CR.hsv8_to_rgb(hsv)


def evaluate(bank, d):
    """One frame from its descriptor (the dict style_morph.plan emits; every weight rounded to fp32 once)."""
    sums = []
    for sd in d["sides"]:
        S = bank[sd["orig"]].astype(f32) * f32(sd["orig_w"])
        for t in sd["terms"]:
            lo = bank[t["lo"]].astype(f32)
            sf = lo if t["hi"] < 0 else lo * f32(t["w_lo"]) + bank[t["hi"]].astype(f32) * f32(t["w_hi"])
            S = S + sf * f32(t["weight"])
        sums.append(S)
    v = sums[0] * f32(d["fade"][0]) + sums[1] * f32(d["fade"][1]) if d["n_sides"] == 2 else sums[0]
    assert v.dtype == f32
    return apply_filter(np.clip(v, 0, 255).astype(np.uint8), d["filter"], d["fparam"])


# ---- the layout the host and the CLI tests share ----
# name -> {family: rungs present}, families in the script's table order.  IMG_001: ladders of 8, 2 and 1 rungs, and its
# second family sits at ladder position exactly 1.0 at global time 0 (sin(pi / 2)); IMG_002 lacks udnie.
LAYOUT = (
    ("IMG_001", {"candy": 8, "udnie": 2, "mosaic": 1}),
    ("IMG_002", {"candy": 8, "mosaic": 2}),
    ("IMG_003", {"candy": 2, "udnie": 1, "tenharmsel": 8}),
)


def layout_images(h, w, seed=5, filters=("vibrance", "warm", "subtle_sat")):
    """render()'s image_data for LAYOUT with random u8 images."""
    rng = np.random.default_rng(seed)

    def img():
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return [dict(name=name, orig=img(), ladders={fam: [img() for _ in range(n)] for fam, n in fams.items()}, filter=flt)
            for (name, fams), flt in zip(LAYOUT, filters)]


def plan_images(image_data):
    """style_morph.plan()'s `images` of a render() image_data."""
    return [dict(families=[(fam, len(v)) for fam, v in d["ladders"].items()], filter=d["filter"]) for d in image_data]


def bank_of(image_data, needs, idx):
    """The bank a frame of still idx reads: needs[idx] followed by needs[idx + 1]."""
    out = []
    for i in (idx, idx + 1):
        if i < len(image_data):
            d = image_data[i]
            out += [d["orig"] if key[0] == "original" else d["ladders"][key[0]][key[1]] for key in needs[i]]
    return np.stack(out)
