"""numpy restatement of the optical-flow morph (neuralstyletransferv1_amd/morph.py) -- TEST INFRASTRUCTURE ONLY.

Written from the reference's scripts (scripts/optical_flow_slideshow.py:17-70, scripts/morph_v2.py:365-468) and from
OpenCV's documented arithmetic, not from the kernels:
  gray_cv          cv2.cvtColor(COLOR_BGR2GRAY) on 8-bit RGB-ordered input: (R*9798 + G*19235 + B*3735 + 16384) >> 15
  pre_blur         cv2.GaussianBlur(gray, (5, 5), 1.0) in fp32 (taps of getGaussianKernel(5, 1.0), REFLECT_101, rows
                   then columns), rounded half-to-even (OpenCV >= 4 uses 8.8 fixed point on u8: may differ by 1 level)
  farneback_gauss  calcOpticalFlowFarneback with OPTFLOW_FARNEBACK_GAUSSIAN: oracle.flow_oracle's pyramid loop, PolyExp
                   and UpdateMatrices with FarnebackUpdateFlow_GaussianBlur's window and fp32 solve
  flow_post        morph_v2.py:405-432 (blur 15x15 sigma 3, radial term where |flow| < 2)
  remap_reflect    cv2.remap(INTER_LINEAR, BORDER_REFLECT) on u8 in the 1/32-pixel fixed point
  add_weighted     cv2.addWeighted on u8
  schedule         the two presets' t / alpha
cv2 is not installed here, so every one of these is PARITY UNPINNED against OpenCV itself.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import flow_oracle as FO

f32 = np.float32
# pyr_scale, levels, winsize, iterations, poly_n, poly_sigma
PRESETS = {
    "slideshow": dict(farneback=(0.5, 5, 15, 3, 7, 1.5), pre_blur=False, post=False),
    "v2": dict(farneback=(0.5, 6, 21, 5, 7, 1.5), pre_blur=True, post=True),
}


def gray_cv(rgb_u8: np.ndarray) -> np.ndarray:
    x = rgb_u8.astype(np.int64)
    return ((x[..., 0] * 9798 + x[..., 1] * 19235 + x[..., 2] * 3735 + 16384) >> 15).astype(np.uint8)


def pre_blur(gray_u8: np.ndarray) -> np.ndarray:
    return np.clip(np.rint(FO.gauss_blur(gray_u8.astype(f32), 5, 1.0)), 0, 255).astype(np.uint8)


def window_taps(winsize: int) -> np.ndarray:
    """k[0..m]: k[0] = 1, k[i] = (float)exp(-i*i / (2 sigma^2)), sigma = m * 0.3; s = 1 + 2 sum k[i] in double;
    k[i] = (float)(k[i] / s)."""
    m = winsize // 2
    sigma = m * 0.3
    k = [f32(1.0)] + [f32(math.exp(-i * i / (2 * sigma * sigma))) for i in range(1, m + 1)]
    s = 1.0 + 2.0 * sum(float(v) for v in k[1:])
    return np.array([f32(float(v) / s) for v in k], dtype=f32)


def blur_solve_gauss(M: np.ndarray, winsize: int) -> np.ndarray:
    """FarnebackUpdateFlow_GaussianBlur: fp32 separable window over the 5 fields (replicated border), fp32 solve."""
    h, w, _ = M.shape
    k = window_taps(winsize)
    m = winsize // 2
    ys, xs = np.arange(h), np.arange(w)
    v = M * k[0]
    for i in range(1, m + 1):
        v = v + (M[np.maximum(ys - i, 0)] + M[np.minimum(ys + i, h - 1)]) * k[i]
    s = v * k[0]
    for i in range(1, m + 1):
        s = s + (v[:, np.maximum(xs - i, 0)] + v[:, np.minimum(xs + i, w - 1)]) * k[i]
    assert s.dtype == f32
    g11, g12, g22, h1, h2 = (s[..., c] for c in range(5))
    idet = f32(1.0) / (g11 * g22 - g12 * g12 + f32(1e-3))
    return np.stack([(g11 * h2 - g12 * h1) * idet, (g22 * h1 - g12 * h2) * idet], -1).astype(f32)


def farneback_gauss(prev: np.ndarray, nxt: np.ndarray, pyr_scale=0.5, levels=5, winsize=15, iterations=3, poly_n=7,
                    poly_sigma=1.5) -> np.ndarray:
    """oracle.flow_oracle.farneback's pyramid loop with the Gaussian window."""
    h, w = prev.shape
    scale, k = 1.0, 0
    while k < levels:
        scale *= pyr_scale
        if w * scale < 32 or h * scale < 32:
            break
        k += 1
    levels = k
    prev_flow = None
    for k in range(levels, -1, -1):
        scale = 1.0
        for _ in range(k):
            scale *= pyr_scale
        sigma = (1.0 / scale - 1) * 0.5
        ksz = max(int(np.rint(sigma * 5)) | 1, 3)
        lw, lh = int(np.rint(w * scale)), int(np.rint(h * scale))
        flow = (np.zeros((lh, lw, 2), dtype=f32) if prev_flow is None
                else FO.resize_lin(prev_flow, lh, lw, 1.0 / pyr_scale))
        R = []
        for img in (prev, nxt):
            b = FO.gauss_blur(img.astype(f32), ksz, sigma)
            if (lh, lw) != (h, w):
                b = FO.resize_lin(b, lh, lw)
            R.append(FO.poly_exp(b, poly_n, poly_sigma))
        M = FO.update_matrices(R[0], R[1], flow)
        for it in range(iterations):
            flow = blur_solve_gauss(M, winsize)
            if it < iterations - 1:
                M = FO.update_matrices(R[0], R[1], flow)
        prev_flow = flow
    return prev_flow


def surviving_levels(h: int, w: int, levels: int, pyr_scale: float = 0.5) -> int:
    scale, k = 1.0, 0
    while k < levels:
        scale *= pyr_scale
        if w * scale < 32 or h * scale < 32:
            break
        k += 1
    return k


def flow_post(flow: np.ndarray, sign: float):
    """morph_v2.py:405-432: sign +1 for the forward flow (+=), -1 for the backward flow (-=).  Returns (flow, the
    blurred flow's magnitude that the threshold looked at)."""
    h, w, _ = flow.shape
    dx = FO.gauss_blur(flow[..., 0], 15, 3.0)
    dy = FO.gauss_blur(flow[..., 1], 15, 3.0)
    mag = np.sqrt(dx * dx + dy * dy)
    assert mag.dtype == f32
    low = mag < f32(2.0)
    rx = (np.arange(w)[None, :] - w / 2.0) / w
    ry = (np.arange(h)[:, None] - h / 2.0) / h
    ox = (dx.astype(np.float64) + sign * rx * 4.0).astype(f32)
    oy = (dy.astype(np.float64) + sign * ry * 4.0).astype(f32)
    return np.stack([np.where(low, ox, dx), np.where(low, oy, dy)], -1).astype(f32), mag


def reflect_index(p, n: int):
    """BORDER_REFLECT (fedcba|abcdefgh|hgfedcba): r = p mod 2n, then r < n ? r : 2n - 1 - r."""
    r = np.mod(p, 2 * n)
    return np.where(r < n, r, 2 * n - 1 - r)


def remap_reflect(img_u8: np.ndarray, mx: np.ndarray, my: np.ndarray) -> np.ndarray:
    """cv2.remap(img, mx, my, INTER_LINEAR, borderMode=BORDER_REFLECT) on u8 [h,w,3]; fp32 maps."""
    h, w, _ = img_u8.shape
    assert mx.dtype == f32 and my.dtype == f32
    with np.errstate(invalid="ignore"):
        mx = np.clip(np.nan_to_num(mx, nan=-2.0 * w, posinf=3.0 * w, neginf=-2.0 * w), -2.0 * w, 3.0 * w).astype(f32)
        my = np.clip(np.nan_to_num(my, nan=-2.0 * h, posinf=3.0 * h, neginf=-2.0 * h), -2.0 * h, 3.0 * h).astype(f32)
    X = np.rint(mx * f32(32)).astype(np.int64)
    Y = np.rint(my * f32(32)).astype(np.int64)
    sx, sy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31
    x0, x1 = reflect_index(sx, w), reflect_index(sx + 1, w)
    y0, y1 = reflect_index(sy, h), reflect_index(sy + 1, h)
    w00, w01 = (32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32
    w10, w11 = (32 - fx) * fy * 32, fx * fy * 32
    assert ((w00 + w01 + w10 + w11) == 32768).all()
    p = img_u8.astype(np.int64)
    acc = (w00[..., None] * p[y0, x0] + w01[..., None] * p[y0, x1] + w10[..., None] * p[y1, x0]
           + w11[..., None] * p[y1, x1])
    return ((acc + 16384) >> 15).astype(np.uint8)


def add_weighted(a_u8: np.ndarray, wa: float, b_u8: np.ndarray, wb: float) -> np.ndarray:
    """cv2.addWeighted(a, wa, b, wb, 0) on u8: fp32 products and sum, rounded half-to-even, saturated."""
    v = a_u8.astype(f32) * f32(wa) + b_u8.astype(f32) * f32(wb)
    assert v.dtype == f32
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def ease_in_out_cubic(t):
    return 4 * t * t * t if t < 0.5 else 1 - pow(-2 * t + 2, 3) / 2


def smoothstep(t):
    return t * t * (3 - 2 * t)


def smootherstep(t):
    return t * t * t * (t * (6 * t - 15) + 10)


def schedule(k: int, preset: str, easing: str = "smooth"):
    """(t, alpha), float64, of the k frames."""
    ease = {"linear": lambda x: x, "smooth": ease_in_out_cubic, "smoother": smootherstep}[easing]
    t, a = [], []
    for i in range(k):
        lin = i / (k - 1) if k > 1 else 0
        if preset == "slideshow":
            t.append(lin)
            a.append(lin)
        else:
            t.append(ease(lin))
            a.append(smoothstep(lin))
    return np.array(t, np.float64), np.array(a, np.float64)


def morph_frames(img1: np.ndarray, img2: np.ndarray, fwd: np.ndarray, bwd: np.ndarray, t, alpha) -> np.ndarray:
    """The frame loop of optical_flow_morph: python-float t times the float32 flow is a float32 product."""
    h, w, _ = img1.shape
    ys, xs = np.mgrid[0:h, 0:w].astype(f32)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for ti, ai in zip(t, alpha):
            w1 = remap_reflect(img1, xs + f32(ti) * fwd[..., 0], ys + f32(ti) * fwd[..., 1])
            w2 = remap_reflect(img2, xs + f32(1 - ti) * bwd[..., 0], ys + f32(1 - ti) * bwd[..., 1])
            out.append(add_weighted(w1, 1 - ai, w2, ai))
    return np.stack(out)


def morph_flows(img1: np.ndarray, img2: np.ndarray, preset: str):
    p = PRESETS[preset]
    g1, g2 = gray_cv(img1), gray_cv(img2)
    if p["pre_blur"]:
        g1, g2 = pre_blur(g1), pre_blur(g2)
    fwd = farneback_gauss(g1, g2, *p["farneback"])
    bwd = farneback_gauss(g2, g1, *p["farneback"])
    if p["post"]:
        fwd, bwd = flow_post(fwd, 1.0)[0], flow_post(bwd, -1.0)[0]
    return fwd, bwd


def optical_flow_morph(img1: np.ndarray, img2: np.ndarray, k: int, preset: str, easing: str = "smooth") -> np.ndarray:
    fwd, bwd = morph_flows(img1, img2, preset)
    t, alpha = schedule(k, preset, easing)
    return morph_frames(img1, img2, fwd, bwd, t, alpha)


def texture_pair(h, w, dx, dy, seed=0):
    """The translated random texture of tests/test_gpu_flow.py's _pair (copied)."""
    rng = np.random.default_rng(seed)
    base = FO.gauss_blur(rng.random((h + 40, w + 40)).astype(np.float32), 9, 2.0)
    base = (base - base.min()) / (base.max() - base.min()) * 255
    prev = np.clip(base[20:20 + h, 20:20 + w], 0, 255).astype(np.uint8)
    nxt = np.clip(base[20 - dy:20 - dy + h, 20 - dx:20 - dx + w], 0, 255).astype(np.uint8)
    return prev, nxt


def post_test_flow(seed: int = 11, n: int = 2, h: int = 64, w: int = 80) -> np.ndarray:
    """The flow of the flow_post tests: random, amplitude +-6, constant over 8 x 8 blocks (white noise of that
    amplitude falls below 2 px everywhere once blurred with sigma 3, and would leave one side of the threshold
    untested)."""
    rng = np.random.default_rng(seed)
    coarse = (rng.random((n, h // 8, w // 8, 2)) - 0.5) * 12
    return np.repeat(np.repeat(coarse, 8, axis=1), 8, axis=2).astype(f32)
