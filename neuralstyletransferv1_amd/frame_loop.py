"""frame_loop.py — the parts of the CLI's frame loop.  pipeline.style_frames builds them and hands the four stage
methods of FrameLoop to frames.run_pipeline (or runs the no-exchange loop over them).  Each part is constructed with
what it needs and owns its own state ("The frame loop's parts"):

    list_frames / check_mask_dir   which frames are styled, under which names (no GPU)
    DecodeAhead                    host decode ahead of the GPU, page-locked staging, H2D       -> (orig, xin)
    Stylizer                       model slots, regions, blend weights                         -> u8 frames | out01 f32
    Masks                          a frame's mask file, the fitted / feathered alphas on the device
    Sink                           D2H on the copy stream, the waiter thread, writers, the files written
    FrameLoop                      stylize_send / root_post / ret_spec / emit: the glue between them

Importing this module loads neither the HIP library nor PIL, torch, regions, temporal or jpegio.
"""
from __future__ import annotations

import contextlib
import os
import re
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional

import numpy as np

FRAME_SUFFIXES = {".png", ".jpg", ".jpeg"}  # pipeline.py:1019-1021
PREFETCH_DEPTH = 2  # shards decoding on the pool beyond the one the GPU is about to take


def _log(msg: str) -> None:
    print(msg, flush=True)


def parse_wh(s) -> Optional[tuple]:
    """'WxH' -> (W, H); None for anything else."""
    m = re.match(r"^\s*(\d+)\s*[xX]\s*(\d+)\s*$", str(s))
    return (int(m.group(1)), int(m.group(2))) if m else None


def frame_number(name: str) -> str:
    """'frame_0012' -> '0012': what a frame's output and mask files are numbered by."""
    return name.split("_")[-1]


# ----------------------------------------------------------------------------- frames in
# EXIF Orientation (tag 0x0112) -> counter-clockwise PIL rotation that uprights the image
_EXIF_UPRIGHT = {3: 180, 6: 270, 8: 90}


def _get_image_with_exif_pil(image_path: str):
    """EXIF-normalised RGB image (pipeline.py:171-187: orientations 3/6/8 rotated upright, others
    untouched; JPEG's legacy _getexif table, absent on other formats)."""
    from PIL import Image
    img = Image.open(image_path)
    tags = getattr(img, "_getexif", lambda: None)() or {}
    angle = _EXIF_UPRIGHT.get(tags.get(0x0112))
    if angle is not None:
        img = img.rotate(angle, expand=True)
    img.load()
    return img if img.mode == "RGB" else img.convert("RGB")  # (convert of an RGB image is a copy)


def _open_rgb(fp):
    """A file (path or open file object), decoded, as an RGB image."""
    from PIL import Image
    im = Image.open(fp)
    im.load()
    return im if im.mode == "RGB" else im.convert("RGB")


class FrameSource:
    """Frames by index: files (PIL decode, optional --inference_res LANCZOS), --input_dir sources staged in memory
    (`staged`: (source path, JPEG quality or None) per frame), or a synthetic stream."""

    def __init__(self, files: Optional[List[Path]] = None, synthetic=None, infer_res: int = 0, staged=None):
        self.files = files if files is not None else ([s for s, _ in staged] if staged is not None else None)
        self.staged = staged
        self.synthetic = synthetic  # (n, h, w)
        self.infer_res = infer_res

    def __len__(self):
        return len(self.files) if self.files is not None else self.synthetic[0]

    def size(self, i: int):
        if self.files is None:
            return (self.synthetic[1], self.synthetic[2])
        from PIL import Image
        with Image.open(self.files[i]) as im:
            w, h = im.size
            if self.staged is not None:  # the staged copy is EXIF-upright: orientations 6 / 8 swap the sides
                try:
                    tags = getattr(im, "_getexif", lambda: None)() or {}
                except Exception:  # noqa: BLE001 -- unreadable EXIF: the raw copy is staged (_open_rgb)
                    tags = {}
                if _EXIF_UPRIGHT.get(tags.get(0x0112)) in (90, 270):
                    w, h = h, w
        return (h, w)

    def _open_rgb(self, i: int):
        if self.staged is None:
            return _open_rgb(self.files[i])
        # the reference's --input_dir staging (pipeline.py:2577-2586): EXIF-upright RGB, re-saved as the staged
        # frame -- PNG (lossless: the decoded frame is that RGB image itself) or JPEG at --jpeg_quality, whose
        # encode -> decode round trip runs here in memory (the same bytes PIL writes, so the same pixels)
        src, q = self.staged[i]
        try:
            pil = _get_image_with_exif_pil(str(src))
        except Exception as e:  # noqa: BLE001 -- pipeline.py:2587-2589: the raw file is copied instead
            _log(f"[stage][WARN] EXIF-normalize failed for {src} ({e}); copying instead")
            return _open_rgb(src)
        if q is None:
            return pil
        # the round trip goes through an anonymous in-memory file with a real descriptor: Pillow encodes to a
        # descriptor with the GIL released (to a BytesIO it holds the GIL, so a thread pool would serialise)
        if hasattr(os, "memfd_create"):
            f = os.fdopen(os.memfd_create("nst_stage"), "w+b")
        else:  # (not Linux: same bytes through a BytesIO)
            import io
            f = io.BytesIO()
        with f:
            pil.save(f, format="JPEG", quality=q)
            f.seek(0)
            return _open_rgb(f)

    def load(self, i: int):
        """-> (original uint8 HxWx3, model-input uint8 hxwx3)."""
        if self.files is None:
            from .synthetic import make_frames
            f = make_frames(1, self.synthetic[1], self.synthetic[2], seed=10_000 + i)[0]
            return f, f
        from PIL import Image
        pil_rgb = self._open_rgb(i)
        pil_src = pil_rgb
        if self.infer_res > 0:  # pipeline.py:1089-1097
            w0, h0 = pil_rgb.size
            m0 = max(w0, h0)
            if m0 > self.infer_res:
                r = self.infer_res / float(m0)
                pil_src = pil_rgb.resize((int(round(w0 * r)), int(round(h0 * r))), Image.Resampling.LANCZOS)
        a = np.asarray(pil_rgb, dtype=np.uint8)
        return a, (a if pil_src is pil_rgb else np.asarray(pil_src, dtype=np.uint8))


def list_frames(args, frames_dir: Optional[Path], stride: int, max_frames: Optional[int]):
    """The frames this run styles -> (FrameSource, their names 'frame_<number>'): a --synthetic stream, the
    --input_dir sources staged in memory (prepare), or the frame_* files of frames_dir."""
    if args.synthetic:
        wh = parse_wh(args.synthetic)
        if not wh:
            _log(f"[error] --synthetic expects WxH, got {args.synthetic}")
            sys.exit(2)
        n_syn = int(args.synthetic_frames)
        if max_frames:
            n_syn = min(n_syn, int(max_frames))
        src = FrameSource(synthetic=(n_syn, wh[1], wh[0]))
        names = [f"frame_{i + 1:04d}" for i in range(n_syn)]
    else:
        staged = getattr(args, "_staged_sources", None)
        if staged is not None:  # frame_{i:04d} of the source's position; only .png/.jpg/.jpeg staged frames are
            # styled (pipeline.py:1019-1021 filters frames_dir by suffix)
            entries = [(f"frame_{i:04d}", s) for i, s in enumerate(staged, start=1)
                       if Path(s[0]).suffix.lower() in FRAME_SUFFIXES]
        else:
            entries = [(p.stem, p) for p in sorted(frames_dir.iterdir()) if p.is_file()
                       and p.name.startswith("frame_") and p.suffix.lower() in FRAME_SUFFIXES]
        if stride and stride > 1:
            entries = entries[::stride]
        if max_frames:
            entries = entries[:max_frames]
        if not entries:
            _log(f"[error] No frames found to style in: {frames_dir}")
            sys.exit(1)
        picked = [e[1] for e in entries]
        src = FrameSource(files=picked if staged is None else None, staged=None if staged is None else picked,
                          infer_res=int(getattr(args, "inference_res", 0) or 0))
        names = [e[0] for e in entries]
    _log(f"[debug] found {len(src)} staged frame(s)")
    return src, names


# ----------------------------------------------------------------------------- masks
def mask_file(args, name: str) -> Optional[str]:
    """The mask file of the frame called `name` (pipeline.py:1985-1993): --mask for every frame, else the
    frame's mask_<number>.png under --mask_dir if it exists; a --synthetic stream looks none up."""
    if getattr(args, "mask", None):
        return args.mask
    if not getattr(args, "mask_dir", None) or args.synthetic:
        return None
    cand = Path(args.mask_dir) / f"mask_{frame_number(name)}.png"
    return str(cand) if cand.exists() else None


def check_mask_dir(args, names: List[str]) -> None:
    """--mask_dir: exit 2 when no frame has a mask there, warn when some lack one."""
    if getattr(args, "mask_dir", None) and not getattr(args, "mask", None) and not args.synthetic:
        md = Path(args.mask_dir)
        missing = sum(1 for nm in names if mask_file(args, nm) is None)
        if missing and missing == len(names):
            _log(f"[mask][ERROR] --mask_dir set to {md} but no masks like mask_0001.png were found.")
            sys.exit(2)
        if missing:
            _log(f"[mask][WARN] {missing}/{len(names)} mask(s) missing under {md}.")


def _pct_to_px(pct: float, H: int) -> int:
    """pipeline.py:278-282."""
    try:
        return int(round(max(0.0, float(pct)) * 0.01 * H))
    except Exception:
        return 0


def load_mask_fit(mask_path: str, target_hw, invert: bool, autofix: bool = True, force_transpose: bool = False) -> np.ndarray:
    """pipeline.py:284-353 without feathering: float32 HxW alpha in [0,1] (host file decode + NEAREST fit)."""
    return load_mask_u8(mask_path, target_hw, invert, autofix, force_transpose).astype(np.float32) / 255.0


def load_mask_u8(mask_path: str, target_hw, invert: bool, autofix: bool = True, force_transpose: bool = False) -> np.ndarray:
    """pipeline.py:292-347: the fitted (and optionally inverted) uint8 mask, before the feather."""
    from PIL import Image
    W_tgt, H_tgt = target_hw[1], target_hw[0]
    m_img = Image.open(mask_path).convert("L")
    mw, mh = m_img.size
    if force_transpose:
        m_img = m_img.transpose(Image.TRANSPOSE)
        mw, mh = m_img.size
    if autofix and (W_tgt != H_tgt):
        reason = None
        if (mw, mh) == (H_tgt, W_tgt):
            reason = "exact-dimension swap"
        else:
            def _dist(a, b):
                return abs(np.log(max(a, 1e-6)) - np.log(max(b, 1e-6)))
            ar_tgt, ar_mask, ar_sw = float(W_tgt) / float(H_tgt), float(mw) / float(mh), float(H_tgt) / float(W_tgt)
            if _dist(ar_mask, ar_sw) + 1e-6 < _dist(ar_mask, ar_tgt):
                reason = "aspect-ratio closer to swapped"
        if reason:
            _log(f"[mask][autofix] {Path(mask_path).name}: {reason}; applying Image.TRANSPOSE")
            m_img = m_img.transpose(Image.TRANSPOSE)
    m_img = m_img.resize((W_tgt, H_tgt), Image.Resampling.NEAREST)
    m = np.array(m_img, dtype=np.uint8)
    if invert:
        m = 255 - m
    return m


class Masks:
    """The frames' alphas on the device; owns the cache of fitted (and feathered) masks by (file, h, w)."""

    def __init__(self, args, names: List[str], dev):
        self.args, self.names, self.dev = args, names, dev
        self.cache: Dict[tuple, object] = {}

    def has(self, f: int) -> bool:  # pipeline.py:1985-1993 mask_used
        return mask_file(self.args, self.names[f]) is not None

    def _alpha(self, mfile: str, h0: int, w0: int):
        import torch
        args = self.args
        key = (mfile, h0, w0)
        if key not in self.cache:
            # pipeline.py:2001-2003: feather radius from --mask_feather_pct of the target height,
            # at least --mask_feather; the Gaussian feather runs on the GPU (nst_mask_feather)
            fpx = _pct_to_px(getattr(args, "mask_feather_pct", 0.0) or 0.0, h0)
            if getattr(args, "mask_feather", 0) and args.mask_feather > 0:
                fpx = max(fpx, int(args.mask_feather))
            m8 = load_mask_u8(mfile, (h0, w0), bool(args.mask_invert), bool(args.mask_autofix),
                              bool(args.mask_force_transpose))
            if fpx > 0:
                from .postproc import feather_masks
                self.cache[key] = feather_masks(torch.from_numpy(m8)[None].to(self.dev), fpx)[0]
            else:
                self.cache[key] = torch.from_numpy(m8.astype(np.float32) / 255.0).to(self.dev)
        return self.cache[key]

    def for_group(self, g: List[int], h0: int, w0: int):
        """float32 [len(g), h0, w0] alphas, or None when no frame of the group has a mask."""
        import torch
        args = self.args
        if not getattr(args, "mask", None) and not getattr(args, "mask_dir", None):
            return None
        files = [mask_file(args, self.names[f]) for f in g]
        if not any(files):
            return None
        # no mask for a frame -> no composite (pipeline.py:1985-1993): the alpha that leaves S unchanged is 1 for
        # 'keep' and 0 for 'replace'
        ident = 1.0 if args.composite_mode == "keep" else 0.0
        return torch.stack([torch.full((h0, w0), ident, dtype=torch.float32, device=self.dev) if m is None
                            else self._alpha(m, h0, w0) for m in files])


# ----------------------------------------------------------------------------- decode-ahead
class PipeProf:
    """Wall time of the frame loop's host-side phases on the main thread (NST_PIPE_PROF=1 prints them)."""

    def __init__(self):
        self.on = os.environ.get("NST_PIPE_PROF", "0") == "1"
        self.t: Dict[str, float] = {}

    @contextlib.contextmanager
    def _timed(self, name: str):
        t0 = time.perf_counter()
        try:
            yield
        finally:
            self.t[name] = self.t.get(name, 0.0) + time.perf_counter() - t0

    def __call__(self, name: str):
        return self._timed(name) if self.on else contextlib.nullcontext()

    def report(self, rank: int):
        if self.on:
            _log(f"[pipe-prof rank {rank}] " + " ".join(f"{k}={v:.3f}s" for k, v in self.t.items()))


class DecodeAhead:
    """Host decode running ahead of the GPU: this rank's next shards are loading on the pool while a shard is
    stylized (and the previous one's encodes drain), so decode, GPU step and encode overlap.  Owns the load futures
    and the page-locked staging of the shards in flight:
      pinned     shard k -> page-locked [n, h, w, 3] the loaders decode into (one H2D copy per shard, async)
      jpeg_recs  --jpeg_reader gpu: shard k -> (page-locked coefficient records [n, record_bytes], JpegInfo); the
                 loaders only entropy-decode, the GPU rebuilds the frames (jpegio.py).  Not with --inference_res
                 (host LANCZOS needs the pixels) or --input_dir staging (EXIF / re-encode round trip): Pillow's"""

    def __init__(self, args, src: FrameSource, sizes, my_shards, pool: ThreadPoolExecutor, prof: PipeProf, dev):
        self.src, self.sizes, self.my_shards, self.pool, self.prof, self.dev = src, sizes, my_shards, pool, prof, dev
        self.shard_pos = {tuple(sh): k for k, sh in enumerate(my_shards) if sh}
        self.loads, self.pinned, self.jpeg_recs = {}, {}, {}
        self.jpeg_gpu = (getattr(args, "jpeg_reader", "pil") == "gpu" and src.files is not None
                         and src.staged is None and src.infer_res == 0)

    def _jpeg_shard(self, sh):
        """the shard's file bytes and common JpegInfo when every frame is a fast-path JPEG of one geometry"""
        from . import jpegio
        if any(Path(self.src.files[f]).suffix.lower() not in (".jpg", ".jpeg") for f in sh):
            return None
        datas, info = [], None
        for f in sh:
            with open(self.src.files[f], "rb") as fh:
                d = fh.read()
            i = jpegio.probe(d)
            if i is None or (info is not None and i != info) or (i.h, i.w) != tuple(self.sizes[f]):
                return None
            info = i
            datas.append(d)
        return datas, info

    def _load_into(self, f, buf, j):
        a, b = self.src.load(f)
        np.copyto(buf[j], a)  # numpy releases the GIL for the copy
        return None if b is a else b

    def _submit(self, k):
        import torch
        if not (0 <= k < len(self.my_shards) and self.my_shards[k] and k not in self.pinned):
            return
        sh, sizes, loads, pool = self.my_shards[k], self.sizes, self.loads, self.pool
        h0, w0 = sizes[sh[0]]
        js = self._jpeg_shard(sh) if self.jpeg_gpu else None
        if js is not None:
            from . import jpegio
            rec = torch.empty((len(sh), js[1].record_bytes), dtype=torch.uint8, pin_memory=True)
            self.pinned[k] = None
            self.jpeg_recs[k] = (rec, js[1])
            rn = rec.numpy()
            for j, f in enumerate(sh):  # -> 0, or a code: the stream is not clean and the shard goes to Pillow
                loads[f] = pool.submit(jpegio.entropy_decode_into, js[0][j], rn[j])
        elif all(sizes[f] == (h0, w0) for f in sh):
            buf = torch.empty((len(sh), h0, w0, 3), dtype=torch.uint8, pin_memory=True)
            self.pinned[k] = buf
            bn = buf.numpy()
            for j, f in enumerate(sh):
                loads[f] = pool.submit(self._load_into, f, bn, j)
        else:
            self.pinned[k] = None
            for f in sh:
                if f not in loads:
                    loads[f] = pool.submit(self.src.load, f)

    def fetch(self, idx: List[int]):
        """The shard's frames on the device -> (orig u8 [n,h0,w0,3], xin u8 [n,h,w,3]: the model's input, `orig`
        itself without --inference_res); submits the next shards' decodes first."""
        import torch
        src, pool, loads, dev = self.src, self.pool, self.loads, self.dev
        k = self.shard_pos.get(tuple(idx), -1)
        for j in range(k, k + 1 + PREFETCH_DEPTH):
            self._submit(j)
        buf = self.pinned.pop(k, None)
        jrec = self.jpeg_recs.pop(k, None)
        with self.prof("wait_decode"):
            loaded = [(loads.pop(f) if f in loads else pool.submit(src.load, f)).result() for f in idx]
            if jrec is not None and any(loaded):  # Pillow warns, raises or decodes the damaged file as it always did
                jrec = None
                loaded = [t.result() for t in [pool.submit(src.load, f) for f in idx]]
        with self.prof("h2d"):
            if jrec is not None:
                from . import jpegio
                orig = xin = jpegio.reconstruct_gpu(jrec[0].to(dev, non_blocking=True), jrec[1])
            elif buf is not None:  # decoded straight into page-locked memory; loaded = the model inputs if different
                orig = buf.to(dev, non_blocking=True)
                xin = orig if loaded[0] is None else torch.from_numpy(np.stack(loaded)).to(dev)
            else:
                orig = torch.from_numpy(np.stack([a for a, _ in loaded])).to(dev, non_blocking=True)
                xin = orig if loaded[0][1] is loaded[0][0] else torch.from_numpy(np.stack([b for _, b in loaded])).to(dev)
        return orig, xin


# ----------------------------------------------------------------------------- stylizer
def _raw_f32(model, preset, xin):
    """One slot's raw output for u8 frames [n,h,w,3]: float32 [n,3,oh,ow], still in the preset's encoding."""
    import torch

    from . import _lib
    n, h, w, _ = xin.shape
    eng = model.engine(xin.device)
    y = torch.empty((n, 3, *eng.output_hw(h, w)), dtype=torch.float32, device=xin.device)
    eng.forward_into(xin, _lib.NST_IO_U8_NHWC, n, h, w, _lib.PRESETS[preset], y, _lib.NST_IO_F32_NCHW)
    return y


def _slot_u8(model, preset, xin, h0, w0):
    """One slot's frames as the reference's to_pil(out.clamp(0,1)): decoded, fitted to the content
    size (bilinear, pipeline.py:1512-1516), clamped, truncated to uint8."""
    import torch

    from . import _lib
    from ._lib import check, lib
    dev = xin.device
    n, h, w, _ = xin.shape
    if model.engine(dev).output_hw(h, w) == (h, w) == (h0, w0):
        return model.stylize_frames(xin, preset)
    y = _raw_f32(model, preset, xin)
    out = torch.empty((n, h0, w0, 3), dtype=torch.uint8, device=dev)
    check(lib().nst_decode_resize_u8(y.data_ptr(), n, y.shape[2], y.shape[3], _lib.PRESETS[preset], out.data_ptr(),
                                     h0, w0, _lib.stream_ptr(dev)), "nst_decode_resize_u8")
    return out


def _blend_slots(slots, weights, xin, h0, w0):
    """Raw f32 outputs of every slot -> nst_blend_models_u8 (decode, fit, weighted sum, clamp, truncation)."""
    import ctypes

    import torch

    from . import _lib
    from ._lib import check, lib
    dev = xin.device
    ys = [_raw_f32(model, preset, xin) for model, preset in slots]
    shapes = {tuple(y.shape) for y in ys}
    if len(shapes) != 1:
        raise _lib.NstError(f"model outputs differ in size {shapes}: the reference cannot blend them either")
    m = len(ys)
    out = torch.empty((xin.shape[0], h0, w0, 3), dtype=torch.uint8, device=dev)
    yp = (ctypes.c_void_p * m)(*[y.data_ptr() for y in ys])
    pr = (ctypes.c_int * m)(*[_lib.PRESETS[preset] for _, preset in slots])
    wt = (ctypes.c_float * m)(*[float(np.float32(w)) for w in weights])
    n, _, oh, ow = ys[0].shape
    check(lib().nst_blend_models_u8(yp, pr, wt, m, n, oh, ow, out.data_ptr(), h0, w0, _lib.stream_ptr(dev)),
          "nst_blend_models_u8")
    return out


class Stylizer:
    """The loaded model slots and how their outputs become one frame: a region composite, the LAB blend, the RGB
    blend, or model A alone.  slots: (model, io_preset) of A and the B..H in use, slot_letters their letter indices;
    n_blend: the models the standard path blends (pipeline.py:1519-1520); weights: the RGB blend's; lab: None or
    (wL, wab, weights of B..) of --blend_models_lab; regions: None or the RegionCompositor."""

    def __init__(self, slots, slot_letters, n_blend: int, weights, lab, regions):
        self.slots, self.slot_letters, self.n_blend = slots, slot_letters, n_blend
        self.weights, self.lab, self.regions = weights, lab, regions

    def __call__(self, xin, orig, fids: List[int], out_f32: bool = False):
        """xin, orig: DecodeAhead.fetch's; fids: the reference's 1-based frame indices (animations, rotation).
        -> the styled frames u8 [n,h0,w0,3] (the reference fits model A's output to the content size), or with
        out_f32 out01 [n,3,h0,w0] float32: the result before the ToPILImage truncation, for the temporal stage."""
        slots, nb, regions = self.slots, self.n_blend, self.regions
        h0, w0 = orig.shape[1], orig.shape[2]
        if regions is not None and regions.optimized:  # crops of the full-resolution frame (pipeline.py:1309)
            return regions.optimized_frames(dict(zip(self.slot_letters, slots)), orig, fids, out_f32=out_f32)
        if regions is not None:
            from .regions import Source, forward_raw
            raw = [Source(forward_raw(m, xin, pr), pr) for m, pr in slots]
            return regions.standard(raw, orig, fids, nb, (h0, w0), out_f32=out_f32)
        if self.lab is not None:  # (only with n_blend > 1; out_f32: to_tensor of the LAB-blended image)
            from .postproc import blend_models_lab
            lab_wl, lab_wab, lab_rest = self.lab
            u8 = blend_models_lab([_slot_u8(m, pr, xin, h0, w0) for m, pr in slots[:nb]], lab_rest, lab_wl, lab_wab)
            if not out_f32:
                return u8
            from .regions import crop_input
            return crop_input(u8, (0, 0, w0, h0), (h0, w0))
        if out_f32:  # model A alone, or the RGB blend: zeros + w_i * out_i, clamp -- one all-ones region
            import torch

            from .regions import Source, composite, forward_raw
            raw = [Source(forward_raw(m, xin, pr), pr) for m, pr in slots[:nb]]
            ones = torch.ones((1, h0, w0), dtype=torch.float32, device=orig.device)
            return composite(raw, [[(i, w) for i, w in enumerate(self.weights[:nb])]], ones, None, out_f32=True)
        if nb == 1 and xin.shape[1:3] == orig.shape[1:3]:
            return slots[0][0].stylize_frames(xin, slots[0][1])
        if nb == 1:
            return _slot_u8(slots[0][0], slots[0][1], xin, h0, w0)
        return _blend_slots(slots[:nb], self.weights, xin, h0, w0)


# ----------------------------------------------------------------------------- sink
@dataclass
class OutputPaths:
    """Where frame f is saved (pipeline.py:2099-2119): its save_map entry in image mode (the suffix decides the
    format), else <prefix>_<number> beside the frames (under --work_dir without a frames_dir)."""
    names: List[str]
    frames_dir: Optional[Path]
    work_dir: str
    prefix: str
    image_ext: str
    image_mode: bool
    save_map: Dict[int, str]

    def __call__(self, f: int):
        """-> (frame f's output file, whether it is a JPEG)"""
        if self.image_mode and (f + 1) in self.save_map:
            out_path = Path(self.save_map[f + 1])
            return out_path, out_path.suffix.lower() in (".jpg", ".jpeg")
        jpg = self.image_ext.lower() == "jpg"
        base = self.frames_dir if self.frames_dir is not None else Path(self.work_dir)
        return (base / f"{self.prefix}_{frame_number(self.names[f])}").with_suffix(".jpg" if jpg else ".png"), jpg


def gpu_writer(args, jpeg_quality: int, jpegs: List[bool]) -> Optional[str]:
    """Which GPU writer builds a group's files, from whether each of its frames is saved as a JPEG: 'png'
    (--png_writer gpu, no --png_compress_level, no JPEG in the group), 'jpeg' (--jpeg_writer gpu, every frame a JPEG,
    at a quality libjpeg takes as given), or None: the host encoders (always with --no_save, which copies pixels)."""
    if args.no_save:
        return None
    if (getattr(args, "png_writer", "pil") == "gpu" and getattr(args, "png_compress_level", None) is None
            and not any(jpegs)):
        return "png"
    if getattr(args, "jpeg_writer", "pil") == "gpu" and 1 <= int(jpeg_quality) <= 100 and all(jpegs):
        return "jpeg"
    return None


def _jpeg_slot_bytes(h: int, w: int) -> int:
    """--jpeg_writer gpu: bytes copied to the host per frame -- the encoder's worst case, but never more than the
    frame's pixels (rounded up to the 16 bytes the encoder wants), so the copy is no larger than without the flag.
    A file that outgrows the slot (nst_jpeg_encode_u8 reports -1) is encoded on the host instead."""
    from .jpegio import jpeg_enc_bound
    return min(jpeg_enc_bound(h, w), (h * w * 3 + 15) // 16 * 16)


class Sink:
    """Finished frames -> files.  Owns the copy stream, the single waiter thread, the hand-offs still waiting for
    their copy (`pending`), the save futures (`saves`) and the list of frames written (`written`)."""

    def __init__(self, args, out_path: OutputPaths, jpeg_quality: int, pool: ThreadPoolExecutor, prof: PipeProf, dev):
        import torch
        self.args, self.out_path, self.jpeg_quality = args, out_path, jpeg_quality
        self.pool, self.prof, self.dev = pool, prof, dev
        self.gpu_flags = "gpu" in (getattr(args, "png_writer", "pil"), getattr(args, "jpeg_writer", "pil"))
        self.copy_stream = torch.cuda.Stream(dev)
        self.waiter = ThreadPoolExecutor(max_workers=1)
        self.pending = []
        self.saves = []  # save futures of handed-off groups, reaped as they finish (errors surface at the next reap)
        self.written: List[int] = []

    def put(self, idx: List[int], styled) -> None:
        """A group's finished frames u8 [n,h,w,3] (frame numbers idx), to be saved behind the GPU's back."""
        import torch
        args, copy_stream = self.args, self.copy_stream
        kind = gpu_writer(args, self.jpeg_quality, [self.out_path(f)[1] for f in idx]) if self.gpu_flags else None
        with self.prof("d2h"):
            # page-locked D2H on a copy stream behind the frames' last kernel; the encoders wait for its event, so
            # this thread goes on queueing the next group's forward instead of waiting for the GPU.  --png_writer gpu
            # and --jpeg_writer gpu: the group's finished files (and their sizes) instead of the pixels
            if kind == "png":
                from .pngio import encode_png_gpu
                src, sizes_d = encode_png_gpu(styled)
            elif kind == "jpeg":
                from . import jpegio
                src, sizes_d = jpegio.encode_jpeg_gpu(styled, int(self.jpeg_quality),
                                                      _jpeg_slot_bytes(styled.shape[1], styled.shape[2]))
            else:
                src, sizes_d = styled, None
            host_t = torch.empty(src.shape, dtype=torch.uint8, pin_memory=True)
            host_sz = torch.empty(src.shape[0], dtype=torch.int64, pin_memory=True) if kind else None
            copy_stream.wait_stream(torch.cuda.current_stream(self.dev))
            with torch.cuda.stream(copy_stream):
                host_t.copy_(src, non_blocking=True)
                if kind:
                    host_sz.copy_(sizes_d, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copy_stream)
            src.record_stream(copy_stream)
            if kind:
                sizes_d.record_stream(copy_stream)
        # one waiter thread per run waits for the copy's event and then hands the frames to the encoder pool, so no
        # pool thread sits blocked on the GPU (the pool also decodes the next groups).  A JPEG group keeps its pixels
        # on the device until then: a frame whose file outgrew the copied slot is saved from them
        self.pending.append(self.waiter.submit(self._hand_off, ev, host_t, list(idx) if not args.no_save else [],
                                               host_sz, styled if kind == "jpeg" else None))
        del host_t  # the waiter holds it until the copy is done; the savers' row views keep it alive after that
        self._reap()
        if not args.no_save:
            self.written.extend(idx)

    def _hand_off(self, ev, host_t, idx, host_sz=None, styled=None):
        import torch
        ev.synchronize()
        host = host_t.numpy()
        # each save holds a row view of the page-locked buffer (numpy keeps the tensor as the view's base), so the
        # buffer is released when the group's last save ends -- not held for the whole run
        if host_sz is None:
            return [self.pool.submit(self._save, host[j], f) for j, f in enumerate(idx)]
        sz = host_sz.tolist()  # finished PNG / JPEG files from the GPU: write their bytes
        futs = []
        for j, f in enumerate(idx):
            if sz[j] >= 0:
                futs.append(self.pool.submit(self._write_file, host[j, :sz[j]], f))
            else:  # the JPEG did not fit its slot (-1): the frame's pixels, encoded on the host as without the flag
                with torch.cuda.stream(self.copy_stream):
                    px = styled[j].cpu().numpy()
                futs.append(self.pool.submit(self._save, px, f))
        return futs

    def _write_file(self, data: np.ndarray, f: int):
        out_path, _ = self.out_path(f)
        out_path.parent.mkdir(parents=True, exist_ok=True)
        with open(out_path, "wb") as fh:
            fh.write(memoryview(data))
        return str(out_path)

    def _save(self, img: np.ndarray, f: int):
        from PIL import Image
        args = self.args
        out_img = Image.fromarray(img)
        out_path, save_as_jpg = self.out_path(f)
        out_path.parent.mkdir(parents=True, exist_ok=True)
        if save_as_jpg:
            out_img.save(out_path, format="JPEG", quality=int(self.jpeg_quality))
        elif getattr(args, "png_compress_level", None) is not None:
            out_img.save(out_path, compress_level=int(args.png_compress_level))
        elif getattr(args, "png_writer", "pil") == "fast":  # same pixels as Pillow's file (pngio docstring)
            from .pngio import write_png
            write_png(out_path, img)
        else:
            out_img.save(out_path)
        return str(out_path)

    def _reap(self, final: bool = False):
        for p in [p for p in self.pending if final or p.done()]:
            self.pending.remove(p)
            self.saves.extend(p.result())
        for q in [q for q in self.saves if final or q.done()]:
            self.saves.remove(q)
            q.result()

    def drain(self) -> None:
        """Wait for every copy and save (their errors surface here), and end the waiter thread."""
        with self.prof("drain_saves"):
            self._reap(final=True)
        self.waiter.shutdown()


# ----------------------------------------------------------------------------- the stages
class FrameLoop:
    """The stages frames.run_pipeline asks for, over the parts above.  The frame's owner stylizes it and, at the
    end, D2Hs and encodes it on its own PCIe link and host pool; the only ordered work is the LAB EMA
    (pipeline.py:1942-1978), which rank 0 runs over the planes it smooths (1 byte per pixel by default) -- or, with
    --flow_ema (`flow` given), the whole temporal chain over [out01 | orig], returning finished frames.  Mask
    composite and blend (pipeline.py:1984-2092) run on the owner."""

    def __init__(self, args, sizes, decode: DecodeAhead, stylizer: Stylizer, masks: Masks, sink: Sink, lab, flow,
                 blend: float, need_orig: bool, total: int, who: str, dev):
        self.args, self.sizes, self.dev = args, sizes, dev
        self.decode, self.stylizer, self.masks, self.sink, self.lab, self.flow = decode, stylizer, masks, sink, lab, flow
        self.blend, self.need_orig, self.total, self.who = blend, need_orig, total, who
        self.ordered_lab = (lab.sl or lab.sc) and flow is None
        self.ordered = bool(self.ordered_lab or flow is not None)  # else: no exchange between the ranks
        self.done = 0
        self.t_start = time.perf_counter()

    def stylize_send(self, idx: List[int]):
        """-> (what goes to rank 0, what stays with the owner): [out01 f32 | orig u8] rows with --flow_ema, else
        the LAB planes to smooth (if any) and the frames [styled | orig if need_orig]."""
        import torch
        flow_mode = self.flow is not None
        if not idx:  # a rank without frames of this group
            h0, w0 = self.sizes[0]
            shape = (0, 15 * h0 * w0) if flow_mode else (0, h0, w0, 6 if self.need_orig else 3)
            full = torch.empty(shape, dtype=torch.uint8, device=self.dev)
        else:
            orig, xin = self.decode.fetch(idx)
            # the temporal stage needs out01 before the ToPILImage truncation (pipeline.py:1884-1943)
            styled = self.stylizer(xin, orig, [f + 1 for f in idx], out_f32=flow_mode)
            n = len(idx)
            full = (torch.cat([styled.view(torch.uint8).reshape(n, -1), orig.reshape(n, -1)], dim=1) if flow_mode
                    else torch.cat([styled, orig], dim=3) if self.need_orig else styled)
        if flow_mode:
            return full, None
        if self.ordered_lab:
            return self.lab.planes(full[..., :3] if self.need_orig else full), full
        return None, full

    def root_post(self, g: List[int], full):
        h0, w0 = self.sizes[g[0]]
        lab, flow = self.lab, self.flow
        if lab.hw is not None and lab.hw != (h0, w0):
            _log(f"[size][reset] frame dims changed {lab.hw} -> {(h0, w0)}; resetting EMA caches")
            lab.reset()
            if flow is not None:
                flow.reset()
        if flow is None:
            return lab.smooth_planes(full, (h0, w0)) if self.ordered_lab else None
        return self._temporal(g, full, h0, w0)

    def _temporal(self, g: List[int], full, h0: int, w0: int):
        """[out01 f32 | orig u8] of a group -> its finished frames: the temporal stage in frame order"""
        import torch

        from .postproc import blend_frames
        from .temporal import motion_alpha, planar_to_u8
        args, lab, blend = self.args, self.lab, self.blend
        nb = 3 * h0 * w0 * 4
        out01 = full[:, :nb].contiguous().view(torch.float32).reshape(len(g), 3, h0, w0)
        orig = full[:, nb:].contiguous().reshape(len(g), h0, w0, 3)
        # None for the first frame of a run (no previous frame); the batch's flows come in one call
        fused, flows = self.flow.batch(out01, orig)
        motion = None
        if getattr(args, "motion_blend", False):  # pipeline.py:2072-2080 alpha from this frame's flow
            motion = [None if fl is None else motion_alpha(fl, blend) for fl in flows]
        styled = lab(planar_to_u8(torch.stack(fused)))
        lab.hw = (h0, w0)
        if self.need_orig:
            styled_in = styled
            styled = blend_frames(styled, orig, blend, self.masks.for_group(g, h0, w0), args.composite_mode)
            if motion is not None:  # frames with a flow and no mask: the motion-adaptive blend replaces it
                for j, f in enumerate(g):
                    if motion[j] is not None and not self.masks.has(f):
                        styled[j:j + 1] = blend_frames(styled_in[j:j + 1], orig[j:j + 1], 1.0, motion[j][None], "keep")
        return styled

    def ret_spec(self, g: List[int]):
        import torch
        h0, w0 = self.sizes[g[0]]
        if self.flow is not None:
            return (h0, w0, 3), torch.uint8
        return ((self.lab.nplanes, h0 * w0), torch.uint8) if self.ordered_lab else None

    def emit(self, idx: List[int], rows, full):
        if not idx:
            return
        if self.flow is not None:
            styled = rows
        else:
            styled = full[..., :3].contiguous() if self.need_orig else full
            if self.ordered_lab:
                styled = self.lab.merge(styled, rows)
            if self.need_orig:
                from .postproc import blend_frames
                h0, w0 = styled.shape[1], styled.shape[2]
                styled = blend_frames(styled, full[..., 3:].contiguous(), self.blend,
                                      self.masks.for_group(idx, h0, w0), self.args.composite_mode)
        self.sink.put(idx, styled)
        self.done += len(idx)
        el = time.perf_counter() - self.t_start
        _log(f"[frame]{self.who} {self.done}/{self.total} styled  ({self.done / max(el, 1e-9):.2f} frames/s)")
