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
