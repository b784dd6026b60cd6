"""GPU JPEG reader (csrc/jpeg_dec.hip behind nst_jpeg_reconstruct_u8, fed by the host entropy decoder): the frames
must equal Pillow's Image.open(f).convert("RGB") (the reference's reader, pipeline.py:1086) byte for
byte, and the CLI with --jpeg_reader gpu must write the files --jpeg_reader pil writes."""
import ctypes
import io

import numpy as np
import pytest
import torch
from PIL import Image

from neuralstyletransferv1_amd import _lib, jpegio, synthetic
from cli_run import run_frames_dir
from jpeg_ref import content, encode, pillow_rgb

pytestmark = pytest.mark.gpu

# (h, w): the smallest shape that reaches each path
SHAPES = [
    (1, 1), (3, 5), (2, 4),  # chroma width <= 2: replication
    (5, 3),                  # ragged, no full block
    (8, 8), (16, 16),        # exactly one block / one MCU
    (17, 33),                # one sample past an MCU both ways
    (24, 40),                # h mod 16 = 8 (the 1080p case): last MCU row half real, bottom-row replication
    (40, 24),                # the same horizontally
    (50, 70),                # the project's ragged shape
    (72, 520),               # several workgroups and the column edges between them
]
QUALITIES = (85, 30, 95)  # frame j of a batch: per-frame tables differ


def _files(h, w, n, mode, **kw):
    out = []
    for j in range(n):
        rgb = content("noise" if j % 2 == 0 else "smooth", h, w, seed=j)
        if mode == "grey":
            b = io.BytesIO()
            Image.fromarray(rgb[..., 1]).save(b, format="JPEG", quality=QUALITIES[j % 3], **kw)
            out.append(b.getvalue())
        else:
            out.append(encode(rgb, quality=QUALITIES[j % 3], subsampling=mode, **kw))
    return out


def _check(files):
    got = jpegio.decode_gpu(files, torch.device("cuda", 0)).cpu().numpy()
    assert got.shape[0] == len(files)
    for j, d in enumerate(files):
        want = pillow_rgb(d)
        assert got[j].shape == want.shape
        assert np.array_equal(got[j], want), (j, int(np.abs(got[j].astype(int) - want).max()))


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("mode", [0, 1, 2, "grey"], ids=["444", "422", "420", "grey"])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_jpeg_equals_pillow(hw, mode, n):
    _check(_files(hw[0], hw[1], n, mode))


@pytest.mark.parametrize("kw", [dict(restart_marker_rows=1), dict(optimize=True)], ids=["restart", "optimize"])
def test_gpu_jpeg_restart_intervals_and_optimized_tables(kw):
    _check(_files(50, 70, 2, 2, **kw))


def test_gpu_jpeg_is_repeatable():
    files = _files(72, 520, 3, 2)
    a = jpegio.decode_gpu(files, torch.device("cuda", 0))
    b = jpegio.decode_gpu(files, torch.device("cuda", 0))
    assert torch.equal(a, b)


def test_decode_gpu_raises_off_the_fast_path():
    good = _files(16, 16, 1, 2)
    with pytest.raises(_lib.NstError):
        jpegio.decode_gpu(good + [encode(content("smooth", 16, 16), progressive=True)], torch.device("cuda", 0))
    with pytest.raises(_lib.NstError):
        jpegio.decode_gpu(good + _files(16, 16, 1, 1), torch.device("cuda", 0))
    with pytest.raises(_lib.NstError):
        jpegio.decode_gpu([good[0][:-40]], torch.device("cuda", 0))


def test_gpu_jpeg_rejects_small_workspace_and_wrong_record_size():
    data = _files(24, 40, 1, 2)[0]
    info = jpegio.probe(data)
    host = np.empty(info.record_bytes, np.uint8)
    assert jpegio.entropy_decode_into(data, host) == 0
    rec = torch.from_numpy(host).cuda()
    L = _lib.lib()
    wsb = ctypes.c_size_t()
    assert L.nst_jpeg_workspace_bytes(1, 24, 40, 3, 2, ctypes.byref(wsb)) == 0
    ws = torch.empty(wsb.value, dtype=torch.uint8, device="cuda")
    out = torch.empty((1, 24, 40, 3), dtype=torch.uint8, device="cuda")
    geo = (1, 24, 40, 3, 2, out.data_ptr(), ws.data_ptr())
    assert L.nst_jpeg_reconstruct_u8(rec.data_ptr(), info.record_bytes, *geo, wsb.value - 1, None) == _lib.NST_E_WORKSPACE
    assert L.nst_jpeg_reconstruct_u8(rec.data_ptr(), info.record_bytes - 128, *geo, wsb.value, None) == _lib.NST_E_INVALID
    assert L.nst_jpeg_reconstruct_u8(rec.data_ptr(), info.record_bytes, *geo, wsb.value, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), pillow_rgb(data))


def _cli(tmp_path, tag, frames_dir, reader, extra, batch=2):
    """the frame loop with this reader -> the bytes of every styled file (all PNG here), in frame order"""
    return list(run_frames_dir(tmp_path, tag, frames_dir, ["--jpeg_reader", reader] + extra, batch).values())


def _frame_dir(tmp_path, variants):
    d = tmp_path / "src_frames"
    d.mkdir()
    frames = synthetic.make_frames(5, 136, 240, seed=41)
    for i, f in enumerate(frames):
        (d / f"frame_{i + 1:04d}.jpg").write_bytes(encode(f, quality=90, **variants.get(i, dict(subsampling=2))))
    return d


@pytest.mark.parametrize("extra", [[], ["--blend", "0.9"]], ids=["lab_smoothing", "blend_need_orig"])
def test_cli_gpu_reader_writes_the_files_the_pillow_reader_writes(tmp_path, extra):
    d = _frame_dir(tmp_path, {})
    assert all(jpegio.probe(p.read_bytes()).sampling == 2 for p in d.iterdir())
    pil = _cli(tmp_path, "pil", d, "pil", extra)
    gpu = _cli(tmp_path, "gpu", d, "gpu", extra)
    assert len(pil) == 5 and pil == gpu


@pytest.mark.parametrize("batch", [2, 3])
def test_cli_gpu_reader_falls_back_per_shard(tmp_path, batch):
    """frame 3 progressive (off the fast path), frame 4 another sampling.  --batch 2: shards (1,2) and (5) take the
    GPU, (3,4) Pillow for the progressive file; --batch 3: (1,2,3) Pillow again, and (4,5) Pillow because its
    geometry is not uniform.  The files still match."""
    d = _frame_dir(tmp_path, {2: dict(subsampling=2, progressive=True), 3: dict(subsampling=0)})
    assert jpegio.probe((d / "frame_0003.jpg").read_bytes()) is None
    assert jpegio.probe((d / "frame_0004.jpg").read_bytes()).sampling == 0
    pil = _cli(tmp_path, "pil", d, "pil", ["--blend", "0.9"], batch)
    gpu = _cli(tmp_path, "gpu", d, "gpu", ["--blend", "0.9"], batch)
    assert len(pil) == 5 and pil == gpu
