"""The reference's soft-blob compositor in numpy, written from scripts/selfstyle_blob.py (create_soft_multi_blob_masks,
get_blended_image, generate_blob_video's loader, frame loop and output size), without cv2: cv2.addWeighted is
morph_ref.add_weighted, cv2.resize is the oracle's cv_resize_linear_u8.

The reference pins numpy < 2.0, where a Python (float64) scalar combined with a float32 array gives a float32 array:
every array operation of the masks is float32 and every scalar is rounded to float32 before it meets the array.  Under
NumPy 2 the same lines would promote to float64, so every scalar here is wrapped in np.float32 explicitly (scalar-only
sub-expressions such as time_offset * (1 + octave * 0.3) and amp * 0.5 stay Python doubles, rounded once) and the
functions compute the reference's values under either NumPy.

libm="numpy" takes float32 np.sin / np.exp; libm="double" evaluates the two functions in float64 and rounds once: the
same arithmetic with a differently rounded library.  The distance between the two is the yardstick for what a third
library, the GPU's, may differ by.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

import morph_ref
from oracle.deeplab_oracle import cv_resize_linear_u8

f32 = np.float32


def _sin(a, libm):
    assert a.dtype == f32
    return np.sin(a) if libm == "numpy" else np.sin(a.astype(np.float64)).astype(f32)


def _exp(a, libm):
    assert a.dtype == f32
    return np.exp(a) if libm == "numpy" else np.exp(a.astype(np.float64)).astype(f32)


def _legacy_draws(seed, count):
    """`count` draws of the legacy global generator after np.random.seed(seed), as the script makes them."""
    np.random.seed(seed)
    return [np.random.random() for _ in range(count)]


def soft_masks(H, W, frame_idx, nb=2, frequency=3.0, speed=1.0, seed=42, feather=0.15, libm="numpy"):
    """create_soft_multi_blob_masks: float32 [nb, H, W] softmax weights of nb sine-noise fields."""
    assert libm in ("numpy", "double")
    pi = f32(np.pi)
    t0 = frame_idx * speed * 0.02                       # a Python double, like every scalar below until it is wrapped
    yn = np.linspace(0, 1, H, dtype=f32).reshape(H, 1)
    xn = np.linspace(0, 1, W, dtype=f32).reshape(1, W)
    fields = np.zeros((nb, H, W), dtype=f32)
    for b in range(nb):
        draws = _legacy_draws(seed + 1000 * b, 12)      # per octave: x, y, t
        bp = f32(b * 2 * np.pi / nb)
        acc = np.zeros((H, W), dtype=f32)
        for o in range(4):
            fr, amp = f32(frequency * (2 ** o)), 1.0 / (1.5 ** o)
            px, py, pt = (f32(d * 2 * np.pi) for d in draws[3 * o:3 * o + 3])
            acc = acc + f32(amp) * _sin(yn * fr * pi + py + f32(t0 * (1 + o * 0.3)) + bp, libm)
            acc = acc + f32(amp) * _sin(xn * fr * pi + px + f32(t0 * (1.2 + o * 0.2)) + bp, libm)
            acc = acc + f32(amp * 0.5) * _sin((xn + yn) * fr * pi + pt + f32(t0 * 1.5) + bp, libm)
        assert acc.dtype == f32
        fields[b] = acc
    T = f32(max(0.1, feather * 5))
    e = _exp((fields - fields.max(axis=0, keepdims=True)) / T, libm)
    weights = e / (e.sum(axis=0, keepdims=True) + f32(1e-6))
    assert weights.dtype == f32
    return weights


def stream_position(t, blob_idx, num_blobs, num_images, transition_speed):
    """(idx1, idx2, 1 - blend, blend) of get_blended_image at the frame loop's position of blob blob_idx."""
    phase_offset = blob_idx / num_blobs
    pos = (t * transition_speed * (num_images - 1) + phase_offset * num_images) % num_images
    pos = pos % num_images
    idx1 = int(pos)
    idx2 = (idx1 + 1) % num_images
    blend = pos - idx1
    return idx1, idx2, 1 - blend, blend


def schedule(n_styled, n_magenta, fps, duration, num_blobs, transition_speed):
    """Per frame and blob ("styled" or "magenta", idx1, idx2, w1, w2): what the frame loop blends."""
    total_frames = fps * duration
    out = []
    for frame_idx in range(total_frames):
        t = frame_idx / total_frames
        row = []
        for blob_idx in range(num_blobs):
            magenta = bool(n_magenta) and blob_idx % 2 == 1
            n = n_magenta if magenta else n_styled
            row.append(("magenta" if magenta else "styled",) + stream_position(t, blob_idx, num_blobs, n, transition_speed))
        out.append(row)
    return out


def blend_frame(imgs, masks):
    """frame = sum_b img_b.astype(float32) * mask_b, in blob order from zeros, .astype(uint8)."""
    frame = np.zeros(imgs[0].shape, dtype=f32)
    for img, m in zip(imgs, masks):
        frame += img.astype(f32) * m[:, :, None]
    assert frame.dtype == f32
    return frame.astype(np.uint8)


def load_and_blend(images, original, blend_original):
    loaded = []
    for img in images:
        if blend_original > 0:
            o = original if img.shape == original.shape else cv_resize_linear_u8(original, img.shape[1], img.shape[0])
            img = morph_ref.add_weighted(img, 1 - blend_original, o, blend_original)
        loaded.append(img)
    return loaded


def output_size(H, W, max_resolution):
    if max(H, W) > max_resolution:
        scale = max_resolution / max(H, W)
        return int(W * scale) - (int(W * scale) % 2), int(H * scale) - (int(H * scale) % 2)
    return W - (W % 2), H - (H % 2)


def render(styled, original, magenta=None, fps=24, duration=30, blend_original=0.5, blob_frequency=2.5, blob_speed=1.0,
           max_resolution=1280, seed=42, num_blobs=2, transition_speed=1.0, feather=0.15, libm="numpy", frames=None):
    """generate_blob_video over decoded u8 RGB images of one size (styled, magenta: lists; original: any size): the
    list of output frames as the script hands them to its writer.  `frames`: only these frame numbers."""
    loaded = {"styled": load_and_blend(styled, original, blend_original),
              "magenta": load_and_blend(magenta, original, blend_original) if magenta else []}
    H, W = loaded["styled"][0].shape[:2]
    new_w, new_h = output_size(H, W, max_resolution)
    out = []
    for frame_idx, row in enumerate(schedule(len(loaded["styled"]), len(loaded["magenta"]), fps, duration, num_blobs,
                                             transition_speed)):
        if frames is not None and frame_idx not in frames:
            continue
        masks = soft_masks(H, W, frame_idx, num_blobs, blob_frequency, blob_speed, seed, feather, libm)
        imgs = [morph_ref.add_weighted(loaded[s][i1], w1, loaded[s][i2], w2) for s, i1, i2, w1, w2 in row]
        frame = blend_frame(imgs, masks)
        out.append(frame if (new_w, new_h) == (W, H) else cv_resize_linear_u8(frame, new_w, new_h))
    return out


def tile_configs(min_tile=256, max_tile=512, num_styles=24):
    """generate_tile_configs: tiles min_tile, min_tile + step, ... with up to three overlaps each (tile // 8 but at
    least 16, the midpoint rounded down to a multiple of 8, tile // 3), cut off at num_styles pairs."""
    step = max(16, (max_tile - min_tile) // max(4, num_styles // 3))
    pairs = []
    for tile in range(min_tile, max_tile + 1, step):
        low, high = max(16, tile // 8), tile // 3
        mid = (low + high) // 2 // 8 * 8
        if high > low + 8 and mid != low:
            pairs += [(tile, low), (tile, mid), (tile, high)]
        elif high > low:
            pairs += [(tile, low), (tile, high)]
        else:
            pairs.append((tile, low))
    return pairs[:num_styles]


def sort_key(p):
    """(tile, overlap) read from the `tileN` and `overlapN` parts of a still's name (0 where a part is absent)."""
    found = {"tile": 0, "overlap": 0}
    for part in Path(p).stem.split("_"):
        for word in found:
            if part.startswith(word):
                found[word] = int(part.replace(word, ""))
                break
    return found["tile"], found["overlap"]
