"""Paths through the CLI's frame loop that no other test walks: --stride / --max_frames, a frame directory of mixed
sizes (the EMA reset), a --mask_dir that lacks some frames' masks, and --no_save.  Every case compares the files of
one run with the files of another run that the loop must treat the same, byte for byte."""
import numpy as np
import pytest
from PIL import Image

from cli_run import run_frames_dir
from jpeg_ref import content, encode

pytestmark = pytest.mark.gpu

HW_A, HW_B = (50, 70), (64, 80)


def _frames(tmp_path, tag, hws, ext="png", jpeg_kw=None):
    """frame_0001.. of the given sizes (noise and smooth alternating) -> the directory"""
    d = tmp_path / tag
    d.mkdir()
    for i, (h, w) in enumerate(hws):
        rgb = content("smooth" if i % 2 else "noise", h, w, seed=i)
        p = d / f"frame_{i + 1:04d}.{ext}"
        if ext == "png":
            Image.fromarray(rgb).save(p)
        else:
            p.write_bytes(encode(rgb, quality=90, **(jpeg_kw or {}).get(i, dict(subsampling=2))))
    return d


def _subset(tmp_path, tag, src, numbers):
    d = tmp_path / tag
    d.mkdir()
    for p in sorted(src.iterdir()):
        if int(p.stem.split("_")[-1]) in numbers:
            (d / p.name).write_bytes(p.read_bytes())
    return d


def test_stride_and_max_frames_style_the_frames_a_directory_of_them_alone_would(tmp_path):
    """five frames, --stride 2 --max_frames 2: frames 1 and 3, and to the LAB EMA the same sequence as a directory
    holding only those two"""
    d = _frames(tmp_path, "five", [HW_A] * 5)
    got = run_frames_dir(tmp_path, "strided", d, ["--stride", "2", "--max_frames", "2"])
    assert sorted(got) == ["styled_frame_0001.png", "styled_frame_0003.png"]
    assert got == run_frames_dir(tmp_path, "alone", _subset(tmp_path, "two", d, {1, 3}), [])


@pytest.mark.parametrize("ext,reader", [("png", "pil"), ("jpg", "gpu")])
def test_a_size_change_resets_the_ema(tmp_path, ext, reader):
    """frames 1, 2 of one size and 3, 4 of another: each pair's files are those of a run over that pair alone.
    The JPEG frame 4 is 4:4:4 beside a 4:2:0 frame 3, so with the GPU reader shard (3, 4) goes back to Pillow for
    its mixed geometry while shard (1, 2) is rebuilt on the GPU"""
    d = _frames(tmp_path, "mixed", [HW_A, HW_A, HW_B, HW_B], ext, {3: dict(subsampling=0)})
    extra = ["--jpeg_reader", reader]
    got = run_frames_dir(tmp_path, "all", d, extra)
    assert sorted(got) == [f"styled_frame_{i:04d}.png" for i in range(1, 5)]
    first = run_frames_dir(tmp_path, "first", _subset(tmp_path, "f12", d, {1, 2}), extra)
    second = run_frames_dir(tmp_path, "second", _subset(tmp_path, "f34", d, {3, 4}), extra)
    assert {**first, **second} == got
    h, w = HW_B
    assert np.asarray(Image.open(tmp_path / "all" / "frames" / "styled_frame_0003.png")).shape == (h, w, 3)


def test_mask_dir_without_a_frames_mask_leaves_that_frame_unchanged(tmp_path):
    d = _frames(tmp_path, "two", [HW_A] * 2)
    md = tmp_path / "masks"
    md.mkdir()
    m = np.zeros(HW_A, np.uint8)
    m[:, HW_A[1] // 2:] = 255
    Image.fromarray(m).save(md / "mask_0001.png")
    common = ["--composite_mode", "keep", "--blend", "1.0", "--no-smooth_lightness"]
    plain = run_frames_dir(tmp_path, "plain", d, common)
    masked = run_frames_dir(tmp_path, "masked", d, common + ["--mask_dir", str(md)])
    assert sorted(masked) == sorted(plain) == ["styled_frame_0001.png", "styled_frame_0002.png"]
    assert masked["styled_frame_0002.png"] == plain["styled_frame_0002.png"]  # the identity alpha
    assert masked["styled_frame_0001.png"] != plain["styled_frame_0001.png"]


def test_no_save_writes_nothing(tmp_path):
    from neuralstyletransferv1_amd import pipeline as P
    d = _frames(tmp_path, "four", [HW_A] * 4)
    assert run_frames_dir(tmp_path, "nosave", d, ["--no_save"]) == {}
    assert P.LAST_RUN_STATS["written"] == []
    assert P.LAST_RUN_STATS["frames"] == 4
