"""Host side of what the still compositors' CLIs share (neuralstyletransferv1_amd/stills.py): the six output flags as
each CLI's parser took them before they moved there, the spelling of each CLI's video flag, the names that stay
importable from their old modules, and the bank wrapper's refusal of a CPU tensor.  No GPU."""
from __future__ import annotations

import pytest
import torch

from neuralstyletransferv1_amd import _lib, camera, morph, multi_model_video, stills, style_morph

# minimal valid argv per CLI, and its default --output_prefix
CLIS = {
    "morph": (morph, ["--images", "a.jpg", "b.jpg", "--output_dir", "out"], "morph_frame"),
    "style_morph": (style_morph, ["--styled_dir", "in", "--output_dir", "out"], "style_morph_frame"),
    "multi_model_video": (multi_model_video, ["--orig_dir", "in", "--styled_udnie", "u", "--output_dir", "out"],
                          "multi_model_frame"),
}
# dest: (default, choices, type), as each of the three parsers spelled them out
OUTPUT_FLAGS = {
    "output_dir": (None, None, str),
    "output_prefix": ("<prefix>", None, str),
    "image_ext": ("png", ["png", "jpg"], None),
    "jpeg_quality": (85, None, int),
    "png_writer": ("pil", ["fast", "pil", "gpu"], None),
    "jpeg_writer": ("pil", ["pil", "gpu"], None),
}


@pytest.mark.parametrize("cli", sorted(CLIS))
def test_output_flags(cli):
    mod, argv, prefix = CLIS[cli]
    ap = mod.build_parser()
    args = ap.parse_args(argv)
    actions = {a.dest: a for a in ap._actions}
    for dest, (default, choices, typ) in OUTPUT_FLAGS.items():
        a = actions[dest]
        assert a.option_strings == [f"--{dest}"]
        assert a.required == (dest == "output_dir")
        assert a.default == (prefix if default == "<prefix>" else default)
        assert (None if a.choices is None else list(a.choices)) == choices
        assert a.type is typ
    assert (args.output_dir, args.output_prefix, args.image_ext, args.jpeg_quality, args.png_writer,
            args.jpeg_writer) == ("out", prefix, "png", 85, "pil", "pil")
    with pytest.raises(SystemExit):
        ap.parse_args([x for x in argv if x not in ("--output_dir", "out")])
    got = ap.parse_args(argv + ["--output_prefix", "p", "--image_ext", "jpg", "--jpeg_quality", "70", "--png_writer",
                                "fast", "--jpeg_writer", "gpu"])
    assert (got.output_prefix, got.image_ext, got.jpeg_quality, got.png_writer, got.jpeg_writer) == \
        ("p", "jpg", 70, "fast", "gpu")


def test_video_flag_spellings():
    mo, sm, mm = (CLIS[k][0].build_parser() for k in ("morph", "style_morph", "multi_model_video"))
    a_mo, a_sm, a_mm = (CLIS[k][1] for k in ("morph", "style_morph", "multi_model_video"))
    assert mo.parse_args(a_mo).output_video is None
    assert mo.parse_args(a_mo + ["--output_video", "v.mp4"]).output_video == "v.mp4"
    with pytest.raises(SystemExit):  # morph has no --output (and the prefix of three flags is ambiguous)
        mo.parse_args(a_mo + ["--output", "v.mp4"])
    assert sm.parse_args(a_sm).output_video is None
    assert sm.parse_args(a_sm + ["--output_video", "v.mp4"]).output_video == "v.mp4"
    assert sm.parse_args(a_sm + ["--output", "v.mp4"]).output_video == "v.mp4"
    assert mm.parse_args(a_mm).output is None
    assert mm.parse_args(a_mm + ["--output", "v.mp4"]).output == "v.mp4"
    assert not hasattr(mm.parse_args(a_mm), "output_video")
    with pytest.raises(SystemExit):
        mm.parse_args(a_mm + ["--output_video", "v.mp4"])


def test_old_names_stay():
    assert morph.FrameWriter is stills.FrameWriter
    assert morph.smoothstep is stills.smoothstep is multi_model_video.smoothstep
    assert morph.ease_in_out_cubic is stills.ease_in_out_cubic is camera.ease_in_out_cubic
    assert style_morph.UsageError is stills.UsageError is multi_model_video.UsageError
    for mod in (style_morph, multi_model_video):
        assert callable(mod.load_resize) and callable(mod.load_bank) and callable(mod.fitted_size)
    assert stills.smoothstep(0.25) == 0.25 * 0.25 * (3 - 2 * 0.25)
    assert stills.ease_in_out_cubic(0.25) == 4 * 0.25 ** 3 and stills.ease_in_out_cubic(0.75) == 1 - pow(0.5, 3) / 2


@pytest.mark.parametrize("mod,name", [(style_morph, "style_morph_frames"), (multi_model_video, "multi_model_frames")])
def test_wrapper_refuses_cpu_tensor(mod, name):
    """The device check comes first and carries the wrapper's own name; no library call is made."""
    bank = torch.zeros((2, 4, 4, 3), dtype=torch.uint8)
    with pytest.raises(_lib.NstError, match=rf"^{name} bank must be a tensor on .* there is no CPU path$"):
        getattr(mod, name)(bank, [])
    with pytest.raises(_lib.NstError, match=rf"^{name} bank must be a tensor on .* there is no CPU path$"):
        getattr(mod, name)(bank.float(), [])
