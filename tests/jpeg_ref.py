"""numpy restatement of the JPEG reconstruction (dequantise, jidctint islow IDCT, range limit, fancy chroma
upsampling, YCbCr -> RGB) that csrc/jpeg_dec.hip runs on the device, applied to a coefficient record written by
nst_jpeg_entropy_decode.  Pillow (libjpeg-turbo defaults) is the judge: tests/test_jpeg_host.py requires this to
equal Image.open(f).convert("RGB") bit for bit, which pins the entropy decoder and the arithmetic without a GPU."""
import io

import numpy as np

QT_BYTES = 384


def geometry(h, w, comps, sampling):
    """-> per component: (blocks per row, block rows, real samples per row, real rows); as csrc/jpeg_common.h"""
    hs, vs = (2 if sampling >= 1 else 1), (2 if sampling == 2 else 1)
    if comps == 1:
        hs = vs = 1
    mcux, mcuy = -(-w // (8 * hs)), -(-h // (8 * vs))
    g = [(mcux * hs, mcuy * vs, w, h)]
    if comps == 3:
        g += [(mcux, mcuy, -(-w // hs), -(-h // vs))] * 2
    return g


def record_bytes(h, w, comps, sampling):
    return QT_BYTES + 128 * sum(bw * bh for bw, bh, _, _ in geometry(h, w, comps, sampling))


def _idct_1d(x, shift):
    """jidctint.c islow: x [..., 8] int32 along the last axis -> [..., 8], descaled by `shift` (round half up)"""
    x = x.astype(np.int32)
    z2, z3 = x[..., 2], x[..., 6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * -15137
    tmp3 = z1 + z2 * 6270
    z2, z3 = x[..., 0], x[..., 4]
    tmp0 = (z2 + z3) << 13
    tmp1 = (z2 - z3) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[..., 7], x[..., 5], x[..., 3], x[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    r = 1 << (shift - 1)
    out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2,
           tmp10 - tmp3]
    return np.stack([(o + r) >> shift for o in out], axis=-1)


def _range_limit(v):
    i = v & 1023
    return np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896))).astype(np.int32)


def _plane(coef, qt, bw, bh):
    """coef int16 [bw*bh, 64], qt uint16 [64] -> samples int32 [bh*8, bw*8]"""
    x = coef.astype(np.int32).reshape(-1, 8, 8) * qt.astype(np.int32).reshape(1, 8, 8)
    cols = _idct_1d(x.transpose(0, 2, 1), 11).transpose(0, 2, 1)  # column pass first
    px = _range_limit(_idct_1d(cols, 18))
    return px.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _h2v1(c):
    ch, cw = c.shape
    if cw <= 2:
        return np.repeat(c, 2, axis=1)
    left = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    right = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    out = np.empty((ch, 2 * cw), np.int32)
    out[:, 0::2] = (3 * c + left + 1) >> 2
    out[:, 1::2] = (3 * c + right + 2) >> 2
    return out


def _h2v2(c):
    ch, cw = c.shape
    if cw <= 2:
        return np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)
    above = np.concatenate([c[:1], c[:-1]], axis=0)
    below = np.concatenate([c[1:], c[-1:]], axis=0)
    out = np.empty((2 * ch, 2 * cw), np.int32)
    for par, far in ((0, above), (1, below)):
        cs = 3 * c + far
        left = np.concatenate([cs[:, :1], cs[:, :-1]], axis=1)
        right = np.concatenate([cs[:, 1:], cs[:, -1:]], axis=1)
        out[par::2, 0::2] = (3 * cs + left + 8) >> 4
        out[par::2, 1::2] = (3 * cs + right + 7) >> 4
    return out


def reconstruct(record, h, w, comps, sampling):
    """record: uint8 array of record_bytes(h, w, comps, sampling) -> uint8 [h, w, 3]"""
    rec = np.ascontiguousarray(record, dtype=np.uint8)
    assert rec.size == record_bytes(h, w, comps, sampling)
    qt = rec[:QT_BYTES].view(np.uint16).reshape(3, 64)
    coef = rec[QT_BYTES:].view(np.int16).reshape(-1, 64)
    planes, off = [], 0
    for c, (bw, bh, pw, ph) in enumerate(geometry(h, w, comps, sampling)):
        p = _plane(coef[off:off + bw * bh], qt[c], bw, bh)[:ph, :pw]  # the grid's padding is never read
        off += bw * bh
        planes.append(p)
    y = planes[0]
    if comps == 1:
        return np.repeat(y[..., None], 3, axis=2).astype(np.uint8)
    up = {0: lambda c: c, 1: _h2v1, 2: _h2v2}[sampling]
    cb, cr = (up(p)[:h, :w] - 128 for p in planes[1:])
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


# ---- inputs the JPEG tests share ----
def content(kind: str, h: int, w: int, seed: int = 0) -> np.ndarray:
    if kind == "noise":
        return np.random.default_rng(seed + 1000 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 5 + yy * 3) % 256, (yy * 7) % 256, (xx * 2 + yy * 11) % 256], axis=2).astype(np.uint8)


def encode(rgb: np.ndarray, **kw) -> bytes:
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, format="JPEG", **kw)
    return b.getvalue()


def pillow_rgb(data: bytes) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
