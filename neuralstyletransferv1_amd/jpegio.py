"""Baseline JPEG reader split between host and GPU (`--jpeg_reader gpu`; SURVEY.md §8(f)4 frame I/O).

The reference extracts video frames as MJPEG and opens each with Pillow (pipeline.py:401-408, :1086).  Here the
host does only the serial half -- marker parse and Huffman decode into a record of quantised coefficients
(csrc/jpeg_entropy.cpp, nst_jpeg_entropy_decode: plain C++, thread-safe, called through ctypes with the GIL
released) -- and the GPU does the arithmetic over every sample: dequantise, islow IDCT, range limit, fancy chroma
upsampling, YCbCr -> RGB, NHWC store (csrc/jpeg_dec.hip, nst_jpeg_reconstruct_u8).  The frames equal Pillow's
`Image.open(f).convert("RGB")` byte for byte (tests/test_jpeg_host.py, tests/test_gpu_jpeg.py).

The fast path takes what ffmpeg and Pillow write by default (include/nst_hip.h "JPEG decode" lists it); `probe`
returns None for every other stream and `entropy_decode_into` returns a non-zero code for a damaged one, and the
caller decodes those with Pillow as before.

The writer (`--jpeg_writer gpu`) has no host half: `encode_jpeg_gpu` builds the reference's output files
(pipeline.py:2099-2113, `out_img.save(out_path, format="JPEG", quality=...)`) whole on the GPU, byte for byte what
Pillow writes (csrc/jpeg_enc.hip, nst_jpeg_encode_u8; tests/test_jpeg_enc_host.py, tests/test_gpu_jpeg_enc.py).
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import numpy as np


class JpegInfo(NamedTuple):
    h: int
    w: int
    comps: int
    sampling: int  # _lib.NST_JPEG_444 / 422 / 420
    record_bytes: int


def probe(data: bytes) -> Optional[JpegInfo]:
    """Geometry of a fast-path JPEG stream (headers only), or None when the stream is not one."""
    from . import _lib
    L = _lib.lib()
    h, w, c, s = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rb = ctypes.c_size_t()
    if not data:
        return None
    rc = L.nst_jpeg_probe(data, len(data), ctypes.byref(h), ctypes.byref(w), ctypes.byref(c), ctypes.byref(s),
                          ctypes.byref(rb))
    return JpegInfo(h.value, w.value, c.value, s.value, rb.value) if rc == _lib.NST_OK else None


def entropy_decode_into(data: bytes, buf: np.ndarray) -> int:
    """Entropy-decode one stream into `buf` (a writable contiguous uint8 array of exactly the probed record_bytes,
    e.g. one row of a page-locked tensor).  -> 0, or the library's negative code (the stream is not clean: decode
    it with Pillow)."""
    from . import _lib
    if buf.dtype != np.uint8 or not buf.flags.c_contiguous or not buf.flags.writeable:
        raise ValueError("entropy_decode_into: need a writable contiguous uint8 buffer")
    return _lib.lib().nst_jpeg_entropy_decode(data, len(data), buf.ctypes.data, buf.size)


_ws = {}  # (device, n, h, w, comps, sampling) -> workspace tensor, reused across shards


def reconstruct_gpu(records, info: JpegInfo):
    """records: uint8 [n, info.record_bytes] on an MI355X (one geometry) -> uint8 [n,h,w,3] on the current stream."""
    import torch

    from . import _lib
    _lib.require_gpu_tensor(records, "reconstruct_gpu records")
    if records.dtype != torch.uint8 or records.dim() != 2 or records.shape[1] != info.record_bytes:
        raise ValueError(f"reconstruct_gpu: need uint8 [n, {info.record_bytes}], got {records.dtype} {tuple(records.shape)}")
    records = records.contiguous()
    n = records.shape[0]
    L = _lib.lib()
    wsb = ctypes.c_size_t()
    _lib.check(L.nst_jpeg_workspace_bytes(n, info.h, info.w, info.comps, info.sampling, ctypes.byref(wsb)),
               "nst_jpeg_workspace_bytes")
    key = (records.device, n, info.h, info.w, info.comps, info.sampling)
    ws = _ws.get(key)
    if ws is None:
        if len(_ws) > 4:
            _ws.clear()
        ws = _ws[key] = torch.empty(wsb.value, dtype=torch.uint8, device=records.device)
    out = torch.empty((n, info.h, info.w, 3), dtype=torch.uint8, device=records.device)
    _lib.check(L.nst_jpeg_reconstruct_u8(records.data_ptr(), info.record_bytes, n, info.h, info.w, info.comps,
                                         info.sampling, out.data_ptr(), ws.data_ptr(), wsb.value,
                                         _lib.stream_ptr(records.device)), "nst_jpeg_reconstruct_u8")
    cur = torch.cuda.current_stream(records.device)
    ws.record_stream(cur)
    records.record_stream(cur)
    return out


def decode_gpu(files, device):
    """JPEG files (bytes) of one geometry -> uint8 [n,h,w,3] on `device`.  No quiet fallback: a stream off the fast
    path, a damaged one or mixed geometry raises (the CLI checks with `probe` first and keeps Pillow for those)."""
    import torch

    from . import _lib
    infos = [probe(d) for d in files]
    if not infos or any(i is None for i in infos):
        raise _lib.NstError("decode_gpu: not a fast-path baseline JPEG: " + _lib.lib().nst_last_error().decode())
    if any(i != infos[0] for i in infos):
        raise _lib.NstError("decode_gpu: the files differ in size, components or sampling")
    info = infos[0]
    host = torch.empty((len(files), info.record_bytes), dtype=torch.uint8, pin_memory=True)
    hn = host.numpy()
    for j, d in enumerate(files):
        _lib.check(entropy_decode_into(d, hn[j]), "nst_jpeg_entropy_decode")
    return reconstruct_gpu(host.to(device, non_blocking=True), info)


# ---- JPEG writer on the GPU (`--jpeg_writer gpu`) ----
_enc_ws = {}  # (device, n, h, w) -> workspace tensor, reused across groups


def jpeg_enc_bound(h: int, w: int) -> int:
    """Worst-case size of one h x w file from the GPU writer (nst_jpeg_enc_bound; a multiple of 16)."""
    from . import _lib
    bound = ctypes.c_size_t()
    _lib.check(_lib.lib().nst_jpeg_enc_bound(h, w, ctypes.byref(bound)), "nst_jpeg_enc_bound")
    return bound.value


def jpeg_enc_workspace_bytes(n: int, h: int, w: int) -> int:
    from . import _lib
    wsb = ctypes.c_size_t()
    _lib.check(_lib.lib().nst_jpeg_enc_workspace_bytes(n, h, w, ctypes.byref(wsb)), "nst_jpeg_enc_workspace_bytes")
    return wsb.value


def encode_jpeg_gpu(frames_u8, quality: int, out_stride: Optional[int] = None):
    """uint8 RGB frames [n,h,w,3] on an MI355X -> (files [n, stride] uint8, sizes [n] int64), both on the device,
    on the current stream: file j is files[j, :sizes[j]] and equals what Pillow's
    Image.fromarray(frame).save(f, format="JPEG", quality=quality) writes (csrc/jpeg_enc.hip, nst_jpeg_encode_u8).
    `out_stride` (a multiple of 16; default the worst case of any content) may be smaller than that bound: a frame
    whose file does not fit gets sizes[j] == -1 and the caller encodes it another way.  No CPU path."""
    import torch

    from . import _lib
    _lib.require_gpu_tensor(frames_u8, "encode_jpeg_gpu frames")
    x = frames_u8
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
        raise ValueError(f"encode_jpeg_gpu: need uint8 [n,h,w,3], got {x.dtype} {tuple(x.shape)}")
    x = x.contiguous()
    n, h, w, _ = x.shape
    L = _lib.lib()
    stride = jpeg_enc_bound(h, w) if out_stride is None else int(out_stride)
    wsb = jpeg_enc_workspace_bytes(n, h, w)
    key = (x.device, n, h, w)
    ws = _enc_ws.get(key)
    if ws is None:
        if len(_enc_ws) > 4:
            _enc_ws.clear()
        ws = _enc_ws[key] = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    files = torch.empty((n, stride), dtype=torch.uint8, device=x.device)
    sizes = torch.empty(n, dtype=torch.int64, device=x.device)
    _lib.check(L.nst_jpeg_encode_u8(x.data_ptr(), n, h, w, int(quality), files.data_ptr(), stride, sizes.data_ptr(),
                                    ws.data_ptr(), wsb, _lib.stream_ptr(x.device)), "nst_jpeg_encode_u8")
    cur = torch.cuda.current_stream(x.device)
    ws.record_stream(cur)
    x.record_stream(cur)
    return files, sizes


def jpeg_bytes_gpu(frames_u8, quality: int) -> list:
    """encode_jpeg_gpu, copied to the host: one bytes object (a complete JPEG file) per frame."""
    files, sizes = encode_jpeg_gpu(frames_u8, quality)
    sz = sizes.cpu().tolist()
    host = files.cpu().numpy()
    return [host[j, :sz[j]].tobytes() for j in range(len(sz))]
