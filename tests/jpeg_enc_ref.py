"""numpy / pure-Python restatement of the baseline JPEG encode that csrc/jpeg_enc.hip runs on the device: colour
conversion, 4:2:0 edge replication and h2v2 downsampling, jfdctint islow FDCT, quantisation, the dummy blocks of the
MCU grid, Huffman coding with the standard tables, 0xFF stuffing, padding and the fixed header.  Pillow
(libjpeg-turbo defaults) is the judge: tests/test_jpeg_enc_host.py requires `encode` to equal
Image.fromarray(rgb).save(f, format="JPEG", quality=q) byte for byte, which pins the arithmetic without a GPU."""
import struct
from typing import NamedTuple

import numpy as np

from jpeg_ref import geometry

# libjpeg jcparam.c: the standard tables in natural (row-major) order
STD_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
            14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
            49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
STD_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
              47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7,
          14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46,
          53, 60, 61, 54, 47, 55, 62, 63]  # zigzag position -> natural index

# ITU-T T.81 Annex K.3: (BITS[1..16], HUFFVAL)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])


class Encoded(NamedTuple):
    data: bytes     # the whole file
    zrl: int        # ZRL (0xF0) symbols emitted
    stuffed: int    # 0x00 bytes inserted after 0xFF
    pad_bits: int   # 1-bits that filled the scan's last byte (0: the scan ended on a byte boundary)


def quant_tables(quality: int):
    """-> (luma, chroma) tables in natural order (jcparam.c jpeg_set_quality, force_baseline)"""
    q = max(1, min(100, int(quality)))
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return [[max(1, min(255, (v * scale + 50) // 100)) for v in t] for t in (STD_LUMA, STD_CHROMA)]


def huff_codes(spec):
    """(BITS, HUFFVAL) -> {symbol: (code, length)} (T.81 Annex C)"""
    bits, vals = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def header(h: int, w: int, quality: int) -> bytes:
    """SOI .. SOS, as libjpeg writes them for a 4:2:0 YCbCr image with the standard tables"""
    out = b"\xff\xd8" + b"\xff\xe0" + struct.pack(">H5sBBBHHBB", 16, b"JFIF\0", 1, 1, 0, 1, 1, 0, 0)
    for i, t in enumerate(quant_tables(quality)):
        out += b"\xff\xdb" + struct.pack(">HB", 67, i) + bytes(t[ZIGZAG[k]] for k in range(64))
    out += b"\xff\xc0" + struct.pack(">HBHHB", 17, 8, h, w, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc_th, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += b"\xff\xc4" + struct.pack(">HB", 19 + len(vals), tc_th) + bytes(bits) + bytes(vals)
    out += b"\xff\xda" + struct.pack(">HB", 12, 3) + bytes([1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    return out


def _fdct_1d(d, first):
    """jfdctint.c islow, one pass over the last axis of d [..., 8] (int64)"""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    sh = 11 if first else 15  # CONST_BITS -/+ PASS1_BITS

    def descale(x, n):
        return (x + (1 << (n - 1))) >> n

    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = descale(t10 + t11, 2), descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = descale(z1 + t13 * 6270, sh)
    o[6] = descale(z1 - t12 * 15137, sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = (descale(t4 + z1 + z3, sh), descale(t5 + z2 + z4, sh), descale(t6 + z2 + z3, sh),
                              descale(t7 + z1 + z4, sh))
    return np.stack(o, axis=-1)


def _planes(rgb):
    """u8 [h,w,3] -> the three sample planes, each padded to its real blocks' extent (steps 1-4)"""
    h, w, _ = rgb.shape
    p = rgb.astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    off = (128 << 16) + 32767
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + off) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + off) >> 16
    pw, ph = -(-w // 2), -(-h // 2)
    ye = np.pad(y, ((0, -h % 8), (0, -w % 8)), mode="edge")
    out = [ye]
    for c in (cb, cr):
        c = np.pad(c, ((0, h % 2), (0, 16 * -(-pw // 8) - w)), mode="edge")  # columns fully, rows to an even count
        s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
        bias = np.tile(np.array([1, 2]), s.shape[1] // 2)
        d = (s + bias[None, :]) >> 2
        out.append(np.pad(d, ((0, -ph % 8), (0, 0)), mode="edge"))
    return out


def coefficients(rgb, quality):
    """-> per component: int [block rows, blocks per row, 64] quantised coefficients in natural order over the MCU
    grid; the grid's dummy blocks (step 7) are left zero here and get their DC in `encode`'s MCU walk"""
    h, w, _ = rgb.shape
    geo = geometry(h, w, 3, 2)
    qts = quant_tables(quality)
    res = []
    for ci, plane in enumerate(_planes(rgb)):
        bw, bh = geo[ci][0], geo[ci][1]
        rh, rw = plane.shape[0] // 8, plane.shape[1] // 8
        blk = (plane - 128).reshape(rh, 8, rw, 8).transpose(0, 2, 1, 3)
        rows = _fdct_1d(blk, True)
        full = _fdct_1d(rows.swapaxes(-1, -2), False).swapaxes(-1, -2).reshape(rh, rw, 64)
        div = 8 * np.array(qts[0 if ci == 0 else 1], np.int64)
        q = np.sign(full) * ((np.abs(full) + div // 2) // div)
        grid = np.zeros((bh, bw, 64), np.int64)
        grid[:rh, :rw] = q
        res.append((grid, rh, rw))
    return res


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()
        self.stuffed = 0

    def put(self, v, n):
        self.acc = (self.acc << n) | (v & ((1 << n) - 1))
        self.n += n
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 0xff
            self.out.append(byte)
            if byte == 0xff:
                self.out.append(0)
                self.stuffed += 1
        self.acc &= (1 << self.n) - 1


def encode(rgb: np.ndarray, quality: int) -> Encoded:
    h, w, _ = rgb.shape
    comps = coefficients(rgb, quality)
    dc_t = [huff_codes(DC_LUMA), huff_codes(DC_CHROMA)]
    ac_t = [huff_codes(AC_LUMA), huff_codes(AC_CHROMA)]
    bw = _Bits()
    zrl = 0
    pred = [0, 0, 0]
    mcux, mcuy = comps[1][0].shape[1], comps[1][0].shape[0]
    for my in range(mcuy):
        for mx in range(mcux):
            last_dc = 0  # DC of the block coded just before in this MCU
            for ci, (grid, rh, rw) in enumerate(comps):
                n = 2 if ci == 0 else 1
                for by in range(my * n, my * n + n):
                    for bx in range(mx * n, mx * n + n):
                        blk = [int(v) for v in grid[by, bx]]
                        if by >= rh or bx >= rw:  # dummy block: all AC zero, DC of the previous block
                            blk = [last_dc] + [0] * 63
                        last_dc = blk[0]
                        t = 0 if ci == 0 else 1
                        diff = blk[0] - pred[ci]
                        pred[ci] = blk[0]
                        nb = abs(diff).bit_length()
                        bw.put(*dc_t[t][nb])
                        if nb:
                            bw.put(diff if diff >= 0 else diff - 1, nb)
                        run = 0
                        for k in range(1, 64):
                            v = blk[ZIGZAG[k]]
                            if v == 0:
                                run += 1
                                continue
                            while run > 15:
                                bw.put(*ac_t[t][0xf0])
                                zrl += 1
                                run -= 16
                            nb = abs(v).bit_length()
                            bw.put(*ac_t[t][(run << 4) | nb])
                            bw.put(v if v >= 0 else v - 1, nb)
                            run = 0
                        if run:
                            bw.put(*ac_t[t][0x00])
    pad = (8 - bw.n) % 8
    if pad:
        bw.put((1 << pad) - 1, pad)
    return Encoded(header(h, w, quality) + bytes(bw.out) + b"\xff\xd9", zrl, bw.stuffed, pad)
