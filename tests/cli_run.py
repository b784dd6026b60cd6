"""The CLI tests' shared run of the frame loop over a directory of frames."""
import shutil
from pathlib import Path

import torch

from neuralstyletransferv1_amd import synthetic


def run_frames_dir(tmp_path, tag, frames_dir, extra, batch=2):
    """the video path's frame loop (pipeline._run_style over work_dir/frames, as pipeline.main runs it after the
    extraction) with the synthetic Johnson checkpoint -> {file name: bytes} of the styled files"""
    from neuralstyletransferv1_amd import pipeline as P
    wd = tmp_path / tag
    fd = wd / "frames"
    shutil.copytree(frames_dir, fd)
    ck = tmp_path / "johnson.pth"
    if not ck.exists():
        torch.save(synthetic.make_state_dict("johnson", 2), ck)
    a = P.build_parser().parse_args(["--input_video", "x", "--output_video", "y", "--work_dir", str(wd), "--model",
                                     str(ck), "--io_preset", "imagenet_255", "--dtype", "bf16", "--batch", str(batch),
                                     "--threads", "2"] + extra)
    a.model_type = "transformer"
    P._run_style(a, fd, Path(ck), {}, False)
    return {p.name: p.read_bytes() for p in sorted(fd.glob("styled_frame_*"))}
