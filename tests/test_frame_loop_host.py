"""The frame loop's pure rules (frame_loop.py): which frames are styled, where a frame is saved, which mask file
belongs to a frame, when a GPU writer takes a group.  No GPU."""
import subprocess
import sys
from pathlib import Path

import pytest

from neuralstyletransferv1_amd import frame_loop as FL
from neuralstyletransferv1_amd import pipeline as P


def _args(*extra):
    return P.build_parser().parse_args(["--model", "m.pth"] + list(extra))


def _touch(d: Path, *names):
    d.mkdir(parents=True, exist_ok=True)
    for n in names:
        (d / n).write_bytes(b"")
    return d


# ---- the frame list ----
def test_frames_dir_scan_filters_by_name_and_suffix_then_stride_then_max(tmp_path, capsys):
    d = _touch(tmp_path / "frames", "frame_0001.png", "frame_0002.JPG", "frame_0003.jpeg", "frame_0004.bmp",
               "frame_0005.png", "styled_frame_0001.png", "frame_0006.png", "frame_0007.png")
    (d / "frame_0008.png").mkdir()
    src, names = FL.list_frames(_args(), d, 1, None)
    assert names == ["frame_0001", "frame_0002", "frame_0003", "frame_0005", "frame_0006", "frame_0007"]
    assert [p.name for p in src.files] == ["frame_0001.png", "frame_0002.JPG", "frame_0003.jpeg", "frame_0005.png",
                                           "frame_0006.png", "frame_0007.png"]
    assert src.staged is None and len(src) == 6
    assert "[debug] found 6 staged frame(s)" in capsys.readouterr().out
    assert FL.list_frames(_args(), d, 2, None)[1] == ["frame_0001", "frame_0003", "frame_0006"]
    assert FL.list_frames(_args(), d, 2, 2)[1] == ["frame_0001", "frame_0003"]
    assert FL.list_frames(_args(), d, 1, 4)[1] == ["frame_0001", "frame_0002", "frame_0003", "frame_0005"]
    assert FL.list_frames(_args("--inference_res", "32"), d, 1, 1)[0].infer_res == 32


def test_staged_sources_keep_the_number_of_their_unfiltered_position(tmp_path):
    a = _args()
    a._staged_sources = [(tmp_path / "a.png", None), (tmp_path / "b.tif", None), (tmp_path / "c.JPEG", 85),
                         (tmp_path / "d.jpg", 85)]
    src, names = FL.list_frames(a, tmp_path / "unused", 1, None)
    assert names == ["frame_0001", "frame_0003", "frame_0004"]
    assert src.staged == [a._staged_sources[0], a._staged_sources[2], a._staged_sources[3]]
    assert src.files == [tmp_path / "a.png", tmp_path / "c.JPEG", tmp_path / "d.jpg"]
    assert FL.list_frames(a, None, 2, 1)[1] == ["frame_0001"]


def test_no_frames_exits_1_and_a_bad_synthetic_exits_2(tmp_path, capsys):
    d = _touch(tmp_path / "frames", "frame_0001.bmp", "other_0001.png")
    with pytest.raises(SystemExit) as e:
        FL.list_frames(_args(), d, 1, None)
    assert e.value.code == 1
    assert f"[error] No frames found to style in: {d}" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:
        FL.list_frames(_args("--synthetic", "64by48"), None, 1, None)
    assert e.value.code == 2
    assert "[error] --synthetic expects WxH, got 64by48" in capsys.readouterr().out


def test_synthetic_stream_is_capped_by_max_frames_only():
    src, names = FL.list_frames(_args("--synthetic", " 64 X 48 ", "--synthetic_frames", "5"), None, 2, 3)
    assert src.synthetic == (3, 48, 64) and src.files is None and src.size(0) == (48, 64)
    assert names == ["frame_0001", "frame_0002", "frame_0003"]


def test_canvas_keeps_its_own_message_and_status(capsys):
    assert P._parse_canvas("1920x1080") == (1920, 1080) and P._parse_canvas(None) is None
    with pytest.raises(SystemExit) as e:
        P._parse_canvas("1920*1080")
    assert e.value.code == 2
    assert "[canvas][ERROR] Expected WxH (e.g., 1920x1080), got: 1920*1080" in capsys.readouterr().out


# ---- the output path ----
def test_output_path(tmp_path):
    names = ["frame_0007", "frame_0009"]
    fd = tmp_path / "frames"
    paths = FL.OutputPaths(names, fd, "wd", "styled_frame", "png", False, {1: "/x/a.jpg"})
    assert paths(0) == (fd / "styled_frame_0007.png", False)  # the save_map counts only in image mode
    paths = FL.OutputPaths(names, fd, "wd", "out", "jpg", False, {})
    assert paths(1) == (fd / "out_0009.jpg", True)
    paths = FL.OutputPaths(names, None, str(tmp_path / "wd"), "styled_frame", "png", False, {})
    assert paths(0) == (tmp_path / "wd" / "styled_frame_0007.png", False)
    paths = FL.OutputPaths(names, fd, "wd", "styled_frame", "png", True, {1: "/x/a.JPG", 2: "/x/b.jpeg", 3: "/x/c"})
    assert paths(0) == (Path("/x/a.JPG"), True) and paths(1) == (Path("/x/b.jpeg"), True)
    paths = FL.OutputPaths(names, fd, "wd", "styled_frame", "jpg", True, {1: "/x/a.png"})
    assert paths(0) == (Path("/x/a.png"), False)  # the suffix decides, not --image_ext
    assert paths(1) == (fd / "styled_frame_0009.jpg", True)  # no entry: the numbered file


# ---- masks ----
def test_mask_file_rule(tmp_path):
    md = _touch(tmp_path / "masks", "mask_0002.png", "mask_0003.jpg")
    names = ["frame_0001", "frame_0002", "frame_0003"]
    a = _args("--mask_dir", str(md))
    assert [FL.mask_file(a, n) for n in names] == [None, str(md / "mask_0002.png"), None]
    m = FL.Masks(a, names, None)
    assert [m.has(f) for f in range(3)] == [False, True, False]
    a = _args("--mask_dir", str(md), "--mask", "one.png")  # --mask wins, for every frame
    assert [FL.mask_file(a, n) for n in names] == ["one.png"] * 3
    assert all(FL.Masks(a, names, None).has(f) for f in range(3))
    a = _args("--mask_dir", str(md), "--synthetic", "8x8")  # a synthetic stream never looks masks up
    assert [FL.mask_file(a, n) for n in names] == [None] * 3
    assert FL.Masks(a, names, None).for_group([0, 1, 2], 8, 8) is None
    assert FL.mask_file(_args("--mask", "one.png", "--synthetic", "8x8"), "frame_0001") == "one.png"
    assert FL.mask_file(_args(), "frame_0002") is None
    assert FL.Masks(_args(), names, None).for_group([0, 1], 8, 8) is None


def test_mask_dir_pre_check(tmp_path, capsys):
    md = _touch(tmp_path / "masks", "mask_0002.png")
    FL.check_mask_dir(_args("--mask_dir", str(md)), ["frame_0001", "frame_0002", "frame_0003"])
    assert f"[mask][WARN] 2/3 mask(s) missing under {md}." in capsys.readouterr().out
    FL.check_mask_dir(_args("--mask_dir", str(md)), ["frame_0002"])
    assert capsys.readouterr().out == ""
    with pytest.raises(SystemExit) as e:
        FL.check_mask_dir(_args("--mask_dir", str(md)), ["frame_0001", "frame_0003"])
    assert e.value.code == 2
    assert f"[mask][ERROR] --mask_dir set to {md} but no masks like mask_0001.png were found." in capsys.readouterr().out
    FL.check_mask_dir(_args("--mask_dir", str(md), "--mask", "one.png"), ["frame_0001"])  # not with --mask
    FL.check_mask_dir(_args("--mask_dir", str(md), "--synthetic", "8x8"), ["frame_0001"])  # nor --synthetic
    assert capsys.readouterr().out == ""


# ---- the writer choice ----
def test_gpu_writer_choice():
    png, jpg, mixed = [False, False], [True, True], [False, True]
    both = ["--png_writer", "gpu", "--jpeg_writer", "gpu"]
    assert FL.gpu_writer(_args(), 85, png) is None and FL.gpu_writer(_args(), 85, jpg) is None
    assert FL.gpu_writer(_args("--png_writer", "fast"), 85, png) is None
    assert FL.gpu_writer(_args(*both), 85, png) == "png"
    assert FL.gpu_writer(_args(*both), 85, jpg) == "jpeg"
    assert FL.gpu_writer(_args(*both), 85, mixed) is None  # a JPEG in the group / not every frame a JPEG
    assert FL.gpu_writer(_args("--png_writer", "gpu"), 85, jpg) is None
    assert FL.gpu_writer(_args("--jpeg_writer", "gpu"), 85, png) is None
    assert FL.gpu_writer(_args(*both, "--png_compress_level", "6"), 85, png) is None
    assert FL.gpu_writer(_args(*both, "--png_compress_level", "6"), 85, jpg) == "jpeg"
    for q, want in ((0, None), (1, "jpeg"), (100, "jpeg"), (101, None)):
        assert FL.gpu_writer(_args(*both), q, jpg) == want
    assert FL.gpu_writer(_args(*both), 0, png) == "png"  # the quality does not concern PNG files
    assert FL.gpu_writer(_args(*both, "--no_save"), 85, png) is None
    assert FL.gpu_writer(_args(*both, "--no_save"), 85, jpg) is None


# ---- imports ----
def test_importing_the_loop_loads_no_codec_device_or_stage_module():
    code = ("import sys; from neuralstyletransferv1_amd import pipeline, frame_loop; "
            "pkg = 'neuralstyletransferv1_amd.'; "
            "bad = [m for m in ('PIL', 'torch', pkg + '_lib', pkg + 'regions', pkg + 'temporal', pkg + 'jpegio', "
            "pkg + 'pngio', pkg + 'postproc', pkg + 'frames') if m in sys.modules]; "
            "assert not bad, bad; assert pipeline.FrameSource is frame_loop.FrameSource")
    repo = str(Path(__file__).resolve().parent.parent)
    r = subprocess.run([sys.executable, "-c", code], cwd=repo, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
