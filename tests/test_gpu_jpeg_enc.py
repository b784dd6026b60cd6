"""GPU JPEG writer (csrc/jpeg_enc.hip behind nst_jpeg_encode_u8): every file must equal what Pillow's
Image.fromarray(frame).save(f, format="JPEG", quality=q) writes (the reference's writer, pipeline.py:2099-2113) byte
for byte, and the CLI with --jpeg_writer gpu must leave the files --jpeg_writer pil leaves."""
import ctypes

import numpy as np
import pytest
import torch

from neuralstyletransferv1_amd import _lib, jpegio
from cli_run import run_frames_dir as _cli
from jpeg_ref import content, encode

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 4), (3, 5), (8, 8), (9, 6), (16, 16), (17, 33), (40, 24), (50, 70), (31, 47)]
QUALITIES = (1, 30, 85, 95, 100)
POISON = 0xA5
GUARD = 4096


def _encode_raw(frames: np.ndarray, q: int, stride=None):
    """nst_jpeg_encode_u8 over poisoned output and workspace buffers, each followed by a guard region
    -> (files [n, stride] on the host, sizes list); asserts both guards untouched"""
    n, h, w, _ = frames.shape
    L = _lib.lib()
    wsb = ctypes.c_size_t()
    assert L.nst_jpeg_enc_workspace_bytes(n, h, w, ctypes.byref(wsb)) == 0
    if stride is None:
        stride = jpegio.jpeg_enc_bound(h, w)
    x = torch.from_numpy(frames).cuda()
    out = torch.full((n * stride + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    ws = torch.full((wsb.value + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    sizes = torch.full((n + 2,), -77, dtype=torch.int64, device="cuda")
    assert out.data_ptr() % 16 == 0 and ws.data_ptr() % 16 == 0
    _lib.check(L.nst_jpeg_encode_u8(x.data_ptr(), n, h, w, q, out.data_ptr(), stride, sizes.data_ptr(), ws.data_ptr(),
                                    wsb.value, _lib.stream_ptr(x.device)), "nst_jpeg_encode_u8")
    torch.cuda.synchronize()
    assert bool((out[n * stride:] == POISON).all()), "bytes written past the last slot"
    assert bool((ws[wsb.value:] == POISON).all()), "bytes written past the workspace"
    assert sizes[n:].tolist() == [-77, -77]
    return out[:n * stride].view(n, stride).cpu().numpy(), sizes[:n].tolist()


def _check(frames: np.ndarray, q: int):
    files, sz = _encode_raw(frames, q)
    for j in range(frames.shape[0]):
        want = encode(frames[j], quality=q)
        assert sz[j] == len(want), (j, sz[j], len(want))
        got = files[j, :sz[j]].tobytes()
        if got != want:
            first = next(i for i in range(len(want)) if got[i] != want[i])
            raise AssertionError(f"frame {j}: first difference at byte {first} of {len(want)}")


@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("q", QUALITIES)
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_jpeg_file_equals_pillows(hw, q, kind):
    rgb = content(kind, *hw)
    assert jpegio.jpeg_bytes_gpu(torch.from_numpy(rgb[None]).cuda(), q) == [encode(rgb, quality=q)]


@pytest.mark.parametrize("q", QUALITIES)
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_jpeg_batch_of_three_different_frames(hw, q):
    frames = np.stack([content("noise", *hw, seed=1), content("smooth", *hw), content("noise", *hw, seed=2)])
    _check(frames, q)


def test_gpu_jpeg_scans_cross_many_workgroups():
    _check(content("noise", 272, 480)[None], 95)  # 3,060 blocks, ~220 KB of scan: every scan loops


def test_gpu_jpeg_overflow_leaves_the_other_frames_alone():
    frames = np.stack([content("smooth", 50, 70), content("noise", 50, 70), content("smooth", 50, 70, seed=1)])
    want = [encode(f, quality=100) for f in frames]
    assert len(want[1]) > len(want[0]) + 64
    stride = (max(len(want[0]), len(want[2])) + 15) // 16 * 16
    assert stride < len(want[1])
    files, sz = _encode_raw(frames, 100, stride)
    assert sz == [len(want[0]), -1, len(want[2])]
    assert files[0, :sz[0]].tobytes() == want[0] and files[2, :sz[2]].tobytes() == want[2]
    assert bool((files[1] == POISON).all()), "the frame that did not fit wrote into its slot"


def test_gpu_jpeg_is_repeatable():
    x = torch.from_numpy(np.stack([content("noise", 72, 520, seed=j) for j in range(3)])).cuda()
    fa, sa = jpegio.encode_jpeg_gpu(x, 85)
    fa, sa = fa.clone(), sa.clone()
    fb, sb = jpegio.encode_jpeg_gpu(x, 85)
    assert torch.equal(sa, sb)
    for j, s in enumerate(sa.tolist()):
        assert torch.equal(fa[j, :s], fb[j, :s])


def test_encode_jpeg_gpu_rejects_other_layouts():
    with pytest.raises(ValueError):
        jpegio.encode_jpeg_gpu(torch.zeros((1, 8, 8, 4), dtype=torch.uint8, device="cuda"), 85)
    with pytest.raises(_lib.NstError):
        jpegio.encode_jpeg_gpu(torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda"), 0)


# ---- the CLI ----
@pytest.fixture()
def frame_dir(tmp_path):
    d = tmp_path / "src_frames"
    d.mkdir()
    for i in range(4):  # frames 1 and 3 noise, 2 and 4 smooth
        (d / f"frame_{i + 1:04d}.jpg").write_bytes(encode(content("smooth" if i % 2 else "noise", 50, 70, seed=i),
                                                          quality=90))
    return d


@pytest.mark.parametrize("reader", ["pil", "gpu"])
def test_cli_gpu_writer_leaves_the_files_the_pillow_writer_leaves(tmp_path, frame_dir, reader):
    common = ["--image_ext", "jpg", "--jpeg_reader", reader]
    pil = _cli(tmp_path, "pil", frame_dir, common + ["--jpeg_writer", "pil"])
    gpu = _cli(tmp_path, "gpu", frame_dir, common + ["--jpeg_writer", "gpu"])
    assert sorted(pil) == [f"styled_frame_{i:04d}.jpg" for i in range(1, 5)]
    assert pil == gpu


def test_cli_png_outputs_ignore_the_flag(tmp_path, frame_dir, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the JPEG writer ran for PNG outputs")
    monkeypatch.setattr(jpegio, "encode_jpeg_gpu", boom)
    pil = _cli(tmp_path, "pil", frame_dir, ["--jpeg_writer", "pil"])
    gpu = _cli(tmp_path, "gpu", frame_dir, ["--jpeg_writer", "gpu"])
    assert sorted(pil) == [f"styled_frame_{i:04d}.png" for i in range(1, 5)]
    assert pil == gpu


def test_cli_frame_that_outgrows_its_slot_is_saved_by_pillow(tmp_path, frame_dir, monkeypatch):
    """the slot patched to hold the smaller files of the run but not the larger: those frames come back as -1 and
    are saved from their pixels; every file still equals the Pillow writer's"""
    from neuralstyletransferv1_amd import frame_loop
    common = ["--image_ext", "jpg", "--jpeg_quality", "100"]
    pil = _cli(tmp_path, "pil", frame_dir, common + ["--jpeg_writer", "pil"])
    lens = sorted(len(b) for b in pil.values())
    assert lens[0] + 16 < lens[-1]
    slot = (lens[0] + 15) // 16 * 16
    calls = []

    def small_slot(h, w):
        calls.append((h, w))
        return slot
    monkeypatch.setattr(frame_loop, "_jpeg_slot_bytes", small_slot)
    seen = []
    real = jpegio.encode_jpeg_gpu

    def recording(frames, quality, out_stride=None):
        files, sizes = real(frames, quality, out_stride)
        seen.extend(sizes.cpu().tolist())
        return files, sizes
    monkeypatch.setattr(jpegio, "encode_jpeg_gpu", recording)
    gpu = _cli(tmp_path, "gpu", frame_dir, common + ["--jpeg_writer", "gpu"])
    assert calls and len(seen) == 4
    assert any(s == -1 for s in seen) and any(s > 0 for s in seen)  # both ways taken
    assert pil == gpu
